"""The face crops of a subject db, decoded once and kept on the device as uint8, and the inputs of FaceIdentifier.train() and of
the facial-ID database gathered from them.

    store = CropStore(ctx, n_slots, image_size, device)               # uint8 [n_slots][S][S][3] on the device
    store.load(paths, slots, pool)                                     # host Huffman decode on the pool, device reconstruct
    x = store.gather(idx)                                              # fv_gather_u8_f32: float32 [n][S][S][3] in [0, 1]

The floats are bit for bit what the reference's sequence makes on the host per file (`imread(f).astype(float32) / 255`,
fi.py:1577), so a training step sees the same inputs; what changes is that a crop is decoded once, not once per triplet it
appears in, and that the training thread decodes nothing.  TripletInputs picks one of two tiers (plan_store): the whole db resident
before the first step, or -- a db beyond the budget -- per batch its distinct crops in one of two transient stores, the next
batch decoded by a loader thread while this one trains."""
import numpy as np
import torch

RESIDENT, PER_BATCH, HOST = 'resident', 'per_batch', 'host'
LOAD_CHUNK_BYTES = 64 << 20      # decoded RGB per chunk of CropStore.load (123 crops at 416; the coefficients take 1-2x as much)


def plan_store(n_crops, image_size, budget_bytes):
    """The tier for a db of n_crops crops of image_size: RESIDENT when all of them, as uint8, fit budget_bytes (a budget of 0 holds
    nothing, not even an empty db), else PER_BATCH."""
    S = int(image_size)
    return RESIDENT if int(budget_bytes) > 0 and int(n_crops) * S * S * 3 <= int(budget_bytes) else PER_BATCH


def batch_slots(rows):
    """Triplet rows (anchor, positive, negative labels) -> (the distinct labels in order of first appearance -- anchors, then
    positives, then negatives --, three int32 arrays): unique[ia[j]] == rows[j][0], likewise ip / in for columns 1 and 2."""
    slot, unique = {}, []
    cols = []
    for c in range(3):
        col = np.empty(len(rows), np.int32)
        for j, t in enumerate(rows):
            if t[c] not in slot:
                slot[t[c]] = len(unique); unique.append(t[c])
            col[j] = slot[t[c]]
        cols.append(col)
    return unique, cols[0], cols[1], cols[2]


def store_budget(hps, device):
    """Bytes a resident store may take: hps['crop_store_mb'] where given (0: nothing is resident), else half of what is free on
    the device now -- the caller has allocated the model's workspace first."""
    if hps.get('crop_store_mb') is not None:
        return int(float(hps['crop_store_mb']) * (1 << 20))
    return torch.cuda.mem_get_info(device)[0] // 2


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


class CropStore(object):
    """uint8 [n_slots][S][S][3] on the device.  `ring`: the PinnedRing the coefficients are decoded into (two stores that
    alternate share one)."""

    def __init__(self, ctx, n_slots, image_size, device, ring=None):
        from .postproc import PinnedRing
        self.ctx, self.S, self.dev = ctx, int(image_size), device
        self.data = torch.empty((max(1, int(n_slots)), self.S, self.S, 3), dtype=torch.uint8, device=device)
        self.ring = PinnedRing(2) if ring is None else ring

    @property
    def slot_bytes(self):
        return self.S * self.S * 3

    # ------------------------------------------------------------------ host half (any thread)
    def decode(self, paths, slots, pool):
        """Read and Huffman-decode the files on `pool` into a pinned slot of the ring -> what stage() takes.  A file the parser
        refuses (PNG, progressive, arithmetic-coded, CMYK, 12-bit) or whose scan is damaged is decoded by Pillow instead, that
        file alone.  ValueError naming the file when its pixels are not S x S."""
        from . import face_identification as fi
        from . import jpeg
        from .face_detection import map_all
        torch.cuda.set_device(self.dev)                  # a loader thread pins memory
        S = self.S
        datas = map_all(pool, _read, paths)
        infos = [jpeg.parse(d) for d in datas]
        while True:
            good = [i for i, info in enumerate(infos) if info is not None]
            for i in good:
                if (infos[i].height, infos[i].width) != (S, S):
                    raise ValueError('%s is %d x %d, the store holds %d x %d crops' % (paths[i], infos[i].height, infos[i].width, S, S))
            plan = jpeg.BatchPlan([infos[i] for i in good])
            for k, i in enumerate(good):
                plan.descs[k].rgb_off = int(slots[i]) * self.slot_bytes
            if not good:
                coefs = None
                break
            coefs = self.ring.take(2 * plan.total_coefs).view(torch.int16)
            view = coefs.numpy()

            def entropy(k):
                info = infos[good[k]]
                try:
                    jpeg.entropy_decode(datas[good[k]], info, view[plan.coef_off[k]:plan.coef_off[k] + int(info.total_coefs)])
                    return True
                except ValueError:
                    return False
            damaged = [good[k] for k, ok in enumerate(map_all(pool, entropy, range(len(good)))) if not ok]
            if not damaged:
                break
            self.ring.untake()                           # rare: lay the chunk out again without the damaged files
            for i in damaged:
                infos[i] = None
        rest = [i for i, info in enumerate(infos) if info is None]
        pixels = map_all(pool, lambda i: fi._imread(paths[i]), rest)
        for i, a in zip(rest, pixels):
            if a.shape != (S, S, 3):
                raise ValueError('%s is %d x %d, the store holds %d x %d crops' % (paths[i], a.shape[0], a.shape[1], S, S))
        return coefs, plan, [(int(slots[i]), a) for i, a in zip(rest, pixels)]

    # ------------------------------------------------------------------ device half (the compute stream)
    def stage(self, decoded):
        """ONE host-to-device copy of the chunk's coefficients and ONE fv_jpeg_reconstruct_batch that writes every crop straight
        into its slot; the Pillow-decoded files are uploaded one by one."""
        from . import jpeg
        coefs, plan, rest = decoded
        if coefs is not None:
            jpeg.reconstruct_batch(self.ctx, plan, coefs.to(self.dev, non_blocking=True), self.dev, rgb=self.data.view(-1))
            self.ring.copied(coefs)
        for slot, a in rest:
            self.data[slot].copy_(torch.from_numpy(np.array(a)))      # a copy: Pillow's array is read-only

    def load(self, paths, slots, pool, chunk_bytes=LOAD_CHUNK_BYTES):
        """Decode `paths` into `slots`, in chunks of at most chunk_bytes of decoded RGB: while the device reconstructs a chunk
        the pool decodes the next one into the ring's other slot."""
        if len(paths) != len(slots) or any(not 0 <= int(s) < self.data.shape[0] for s in slots):
            raise ValueError('CropStore.load: one slot in [0, %d) per file' % self.data.shape[0])
        step = max(1, int(chunk_bytes) // self.slot_bytes)
        for i in range(0, len(paths), step):
            self.stage(self.decode(paths[i:i + step], slots[i:i + step], pool))

    def gather(self, idx, out=None):
        from .face_identification import gather_crops_f32
        return gather_crops_f32(self.ctx, self.data, idx, out)


def check_sizes(paths, image_size, pool):
    """ValueError naming the first file whose header gives another size than image_size x image_size (the pixels are not decoded)."""
    from .face_detection import map_all
    from .face_identification import image_hw
    S = int(image_size)
    for p, hw in zip(paths, map_all(pool, image_hw, paths)):
        if tuple(hw) != (S, S):
            raise ValueError('%s is %d x %d, the store holds %d x %d crops' % (p, hw[0], hw[1], S, S))


class TripletInputs(object):
    """The inputs of FaceIdentifier.train()'s steps from a CropStore.  path_of: label -> file; labels: every label a triplet
    may name.  Build it once the training workspace exists (store_budget)."""

    def __init__(self, ctx, device, image_size, labels, path_of, batch_size, budget_bytes, threads, slots=None, tier=None):
        """slots: crops one batch may hold in the per-batch tier (default: the 3 * batch_size of a triplet batch).  tier=HOST: no
        store at all -- crop_batches reads the files on the host, as the sequence's load() does (hps['crop_store'] off)."""
        from concurrent.futures import ThreadPoolExecutor
        from .postproc import PinnedRing
        self.ctx, self.dev, self.S, self.path_of = ctx, device, int(image_size), path_of
        self.tier = plan_store(len(labels), image_size, budget_bytes) if tier is None else tier
        self.pool = ThreadPoolExecutor(max_workers=max(1, int(threads)))
        try:
            if self.tier == HOST:
                pass
            elif self.tier == RESIDENT:
                self.slot_of = {label: k for k, label in enumerate(labels)}
                self.store = CropStore(ctx, len(labels), image_size, device)
                self.store.load([path_of(label) for label in labels], list(range(len(labels))), self.pool)
            else:
                check_sizes([path_of(label) for label in labels], image_size, self.pool)
                ring = PinnedRing(2)
                self.stores = [CropStore(ctx, 3 * int(batch_size) if slots is None else int(slots), image_size, device, ring) for _ in range(2)]
        except Exception:
            self.close()
            raise

    def close(self):
        self.pool.shutdown(wait=True)

    def _split(self, x, n):
        return x[:n], x[n:2 * n], x[2 * n:]

    def batches(self, batches_of_rows):
        """Generator: (xa, xp, xn) of every batch of triplet rows, in order -- three contiguous views of the one [3n][S][S][3]
        tensor a single fv_gather_u8_f32 call wrote."""
        if self.tier == RESIDENT:
            for rows in batches_of_rows:
                idx = [self.slot_of[t[c]] for c in range(3) for t in rows]
                yield self._split(self.store.gather(idx), len(rows))
            return

        def decode(k):
            unique, ia, ip, in_ = batch_slots(batches_of_rows[k])
            store = self.stores[k % 2]
            return store.decode([self.path_of(label) for label in unique], list(range(len(unique))), self.pool), (ia, ip, in_)
        for store, idx, rows in self._ring_batches(decode, batches_of_rows):
            yield self._split(store.gather(np.concatenate(idx)), len(rows))

    def crop_batches(self, batches_of_labels):
        """Generator: one [n][S][S][3] tensor per batch of labels (distinct within a batch), in order, for a step that embeds
        every crop once.  Resident: one fv_gather_u8_f32; per batch: the two ring stores, the next batch decoding meanwhile;
        HOST: the files read on the host, uint8 (the model divides by 255, the same floats)."""
        if self.tier == HOST:
            from .face_identification import _imread
            for batch in batches_of_labels:
                yield np.asarray([_imread(self.path_of(label)) for label in batch])
            return
        if self.tier == RESIDENT:
            for batch in batches_of_labels:
                yield self.store.gather([self.slot_of[label] for label in batch])
            return

        def decode(k):
            batch = batches_of_labels[k]
            if len(batch) > self.stores[k % 2].data.shape[0]:
                raise ValueError('a batch of %d crops, the per-batch stores hold %d' % (len(batch), self.stores[k % 2].data.shape[0]))
            return self.stores[k % 2].decode([self.path_of(label) for label in batch], list(range(len(batch))), self.pool), len(batch)
        for store, n, _batch in self._ring_batches(decode, batches_of_labels):
            yield store.gather(np.arange(n, dtype=np.int32))

    def _ring_batches(self, decode, batches):
        """Generator over the per-batch tier: decode(k) runs on a loader thread one batch ahead -> (the store batch k was staged
        in, what decode returned beside the decoded chunk, batches[k])."""
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=1) as one:          # one-deep prefetch, as FaceDetector._detect_files
            pending = one.submit(decode, 0) if batches else None
            for k, rows in enumerate(batches):
                decoded, more = pending.result()
                if k + 1 < len(batches):
                    pending = one.submit(decode, k + 1)
                # store k % 2 was last read by the gather of batch k - 2, enqueued on this stream before this staging
                store = self.stores[k % 2]
                store.stage(decoded)
                yield store, more, rows
