"""numpy restatement of fv_gather_u8_f32's contract (test aid): slot idx[j] of a uint8 store as row j of a float32 batch, every
byte divided by 255 in IEEE float32 -- what the reference's triplet sequence computes per file on the host (fi.py:1577)."""
import numpy as np


def gather_u8_f32(store, idx):
    """store: uint8 array [n_slots][...]; idx: integer sequence -> float32 [len(idx)][...]"""
    store = np.asarray(store)
    assert store.dtype == np.uint8
    return store[np.asarray(idx, np.int64)].astype(np.float32) / np.float32(255.0)
