"""The FaceIdentifier data mode on one GPU: create_db_fi on seeded synthetic trees shaped like UCCS (18-megapixel frames, several
faces each) and like VGGFace2 (small images, one face each), image_size 416.

For each tree, one batch at a time and every stage on its own (a synchronise between stages, so nothing overlaps): Huffman decode
on the host threads, host-to-device copy + fv_jpeg_reconstruct_batch, the fv_crop_nearest_u8 call, the device-to-host copy of the
crops, Pillow encode + write -- and, next to those two, the device encode of the same crops (jpeg.encode_batch: both calls, the copy
of the byte counts and the device-to-host copy of the files, between device events) and the write of its files.  Then the whole mode as a user runs it (create_db_fi, stages overlapped) in crops/s, with hps.device_encode off and on, alternating with each other and with
the reference's way on the host -- one Pillow decode of the whole image per csv row, a numpy nearest-neighbour gather, one Pillow
save, single-threaded as the reference's UCCS loop is -- run on the first --host-rows rows and extrapolated to the tree when the
tree has more (the JSON says which: host_rows_run < crops means extrapolated).  The crop kernel is also timed alone (device events,
repeated) against its byte floor: bytes written plus the source rows it touches, over the device-to-device copy bandwidth measured
in the same process.  Prints one JSON line.

    python tools/create_db_bench.py [--frames N] [--faces N] [--images N] [--reps N] [--host-rows N]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from face_vijnana_yolov3_amd import face_identification as fi  # noqa: E402
from face_vijnana_yolov3_amd import jpeg  # noqa: E402
from face_vijnana_yolov3_amd._lib import Context  # noqa: E402
from face_vijnana_yolov3_amd.data import letterbox_geometry  # noqa: E402
from face_vijnana_yolov3_amd.face_detection import default_loader_threads  # noqa: E402
from face_vijnana_yolov3_amd.postproc import PinnedRing  # noqa: E402

S = 416


def save_image(path, h, w, rng):
    from PIL import Image
    base = rng.integers(0, 256, (h // 16 + 1, w // 16 + 1, 3)).astype(np.uint8)
    Image.fromarray(np.kron(base, np.ones((16, 16, 1), np.uint8))[:h, :w]).save(path, quality=90)


def uccs_tree(root, frames, faces, rng):
    h, w = 3456, 5184
    os.makedirs(os.path.join(root, 'training'))
    rows = ['FACE_ID,FILE,SUBJECT_ID,FACE_X,FACE_Y,FACE_WIDTH,FACE_HEIGHT']
    for f in range(frames):
        save_image(os.path.join(root, 'training', 'frame_%04d.jpg' % f), h, w, rng)
    k = 0
    for j in range(faces):                       # a frame's rows lie apart in the csv, as in a file sorted by face id
        for f in range(frames):
            fw, fh = rng.uniform(40, 220, 2)
            rows.append('%d,frame_%04d.jpg,%d,%.1f,%.1f,%.1f,%.1f' % (k, f, 1 + k % 97, rng.uniform(1, w - fw - 1),
                                                                      rng.uniform(1, h - fh - 1), fw, fh))
            k += 1
    open(os.path.join(root, 'training', 'training.csv'), 'w').write('\n'.join(rows) + '\n')


def vgg_tree(root, images, rng):
    rows = ['NAME_ID,X,Y,W,H']
    for k in range(images):
        identity = 'n%06d' % (k // 8)
        os.makedirs(os.path.join(root, 'train', identity), exist_ok=True)
        h, w = int(rng.integers(200, 420)), int(rng.integers(180, 380))
        save_image(os.path.join(root, 'train', identity, '%04d_01.jpg' % k), h, w, rng)
        bw, bh = int(rng.integers(80, w - 20)), int(rng.integers(90, h - 20))
        rows.append('%s/%04d_01,%d,%d,%d,%d' % (identity, k, rng.integers(0, w - bw), rng.integers(0, h - bh), bw, bh))
    open(os.path.join(root, 'loose_bb_train.csv'), 'w').write('\n'.join(rows) + '\n')


def conf_of(root, resource_type, device_encode=False):
    return {'fi_conf': dict(mode='data', resource_type=resource_type, raw_data_path=root, nn_arch=dict(image_size=S, dense1_dim=64),
                            hps={'device_encode': device_encode})}


def device_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def copy_bandwidth():
    a = torch.empty(1 << 28, dtype=torch.float32, device='cuda')
    b = torch.empty_like(a)
    for _ in range(2):
        b.copy_(a)
    _, ms = device_ms(lambda: [b.copy_(a) for _ in range(10)])
    return 2 * a.numel() * 4 * 10 / (ms * 1e-3)


def stages(ctx, records, out_dir, threads, bw, iters):
    """Every stage of cut_and_write on its own, batch by batch -> seconds per stage, and the crop kernel against its floor."""
    dev = torch.device('cuda', 0)
    sizes = {}

    def hw_of(p):
        if p not in sizes:
            sizes[p] = fi.image_hw(p)
        return sizes[p]
    ring = PinnedRing(3)
    host = torch.empty((fi.DATA_BATCH_CROPS, S, S, 3), dtype=torch.uint8).pin_memory()
    with ThreadPoolExecutor(max_workers=threads) as pool:
        for timed in (False, True):              # the first pass page-locks the ring, loads code objects and warms the page cache
            t = dict(huffman=0.0, h2d_reconstruct=0.0, crop=0.0, d2h=0.0, encode_write=0.0, device_encode=0.0, write_files=0.0)
            kernel_ms = floor_bytes = file_bytes = 0.0
            for batch in fi.source_batches(records, hw_of):
                t0 = time.perf_counter()
                loaded = fi.load_batch([s for s, _ in batch], pool, ring)
                t['huffman'] += time.perf_counter() - t0
                assert isinstance(loaded[0], str), 'the synthetic trees are baseline JPEGs'
                images, ms = device_ms(lambda: fi.stage_batch(ctx, loaded, ring, dev))
                t['h2d_reconstruct'] += ms * 1e-3
                idx = [i for _, ii in batch for i in ii]
                crops = [(f,) + tuple(records[i].rect) for f, (_, ii) in enumerate(batch) for i in ii]
                if len(crops) > host.shape[0]:
                    host = torch.empty((len(crops), S, S, 3), dtype=torch.uint8).pin_memory()
                cut, ms = device_ms(lambda: fi.crop_nearest_u8(ctx, images, crops, S))
                t['crop'] += ms * 1e-3
                if timed:
                    _, ms = device_ms(lambda: [fi.crop_nearest_u8(ctx, images, crops, S, out=cut) for _ in range(iters)])
                    kernel_ms += ms / iters
                    for _, _y0, _x0, h, w in crops:
                        _w_p, h_p = letterbox_geometry(h, w, S)[:2]
                        floor_bytes += 3.0 * S * S + 3.0 * w * min(h, h_p)
                _, ms = device_ms(lambda: host[:len(crops)].copy_(cut, non_blocking=True))
                t['d2h'] += ms * 1e-3
                pixels = host.numpy()
                t0 = time.perf_counter()
                list(pool.map(lambda ji: fi.write_crop(pixels[ji[0]], os.path.join(out_dir, records[ji[1]].name)), enumerate(idx)))
                t['encode_write'] += time.perf_counter() - t0
                files, ms = device_ms(lambda: jpeg.encode_batch(ctx, cut.view(-1), [j * S * S * 3 for j in range(len(crops))],
                                                                [S, S] * len(crops), dev))
                t['device_encode'] += ms * 1e-3
                file_bytes += sum(len(f) for f in files)
                t0 = time.perf_counter()
                list(pool.map(lambda ji: fi.write_bytes(files[ji[0]], os.path.join(out_dir, records[ji[1]].name)), enumerate(idx)))
                t['write_files'] += time.perf_counter() - t0
    res = {'stage_%s_s' % k: v for k, v in t.items()}
    res.update(crop_kernel_ms=kernel_ms, crop_kernel_floor_ms=floor_bytes / bw * 1e3, file_bytes=file_bytes)
    return res


def host_way(records, out_dir, rows):
    """The reference's loop on the host for the first `rows` records -> seconds."""
    from PIL import Image
    t0 = time.perf_counter()
    for r in records[:rows]:
        img = fi._imread(r.source)                           # the whole image, once per csv row
        y0, x0, h, w = r.rect
        w_p, h_p, pad_t, _pb, pad_l, _pr = letterbox_geometry(h, w, S)
        ys = np.minimum(np.floor(np.arange(h_p) * (1.0 / (h_p / float(h)))).astype(np.int64), h - 1)
        xs = np.minimum(np.floor(np.arange(w_p) * (1.0 / (w_p / float(w)))).astype(np.int64), w - 1)
        out = np.zeros((S, S, 3), np.uint8)
        out[pad_t:pad_t + h_p, pad_l:pad_l + w_p] = img[y0:y0 + h, x0:x0 + w][ys][:, xs]
        Image.fromarray(out).save(os.path.join(out_dir, r.name))
    return time.perf_counter() - t0


def run_tree(tag, root, resource_type, ctx, bw, a):
    enumerate_records = fi.uccs_records if resource_type == 'uccs' else fi.vggface2_records
    records, _ = enumerate_records(root, S)
    n = len(records)
    threads = default_loader_threads()
    scratch = os.path.join(root, 'bench_out')
    os.makedirs(scratch)
    res = {'crops': n, 'loader_threads': threads}
    res.update(stages(ctx, records, scratch, threads, bw, a.iters))
    cwd = os.getcwd()
    os.chdir(root)
    try:
        fi.create_db_fi(conf_of(root, resource_type))            # warm-up: pinned buffers, code objects, the page cache
        rows = min(n, a.host_rows)
        fi.create_db_fi(conf_of(root, resource_type, True))
        dev_s, enc_s, host_s = [], [], []
        for _ in range(a.reps):                                 # alternating
            t0 = time.perf_counter()
            fi.create_db_fi(conf_of(root, resource_type))
            dev_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            fi.create_db_fi(conf_of(root, resource_type, True))
            enc_s.append(time.perf_counter() - t0)
            host_s.append(host_way(records, scratch, rows))
    finally:
        os.chdir(cwd)
    res.update(create_db_fi_s=min(dev_s), create_db_fi_s_all=dev_s, crops_per_s=n / min(dev_s), host_rows_run=rows,
               device_encode_create_db_fi_s_all=enc_s, device_encode_crops_per_s=n / min(enc_s),
               host_loop_s_all=host_s, host_loop_crops_per_s=rows / min(host_s), host_loop_s_for_tree=min(host_s) * n / rows)
    shutil.rmtree(scratch)
    return {'%s_%s' % (tag, k): v for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=12)
    ap.add_argument('--faces', type=int, default=8)
    ap.add_argument('--images', type=int, default=768)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--host-rows', type=int, default=24)
    a = ap.parse_args()
    ctx = Context(0)
    bw = copy_bandwidth()
    res = {'device': torch.cuda.get_device_name(0), 'image_size': S, 'copy_GBps': bw / 1e9}
    tmp = tempfile.mkdtemp()
    try:
        rng = np.random.default_rng(0)
        uccs_tree(os.path.join(tmp, 'uccs'), a.frames, a.faces, rng)
        res.update(run_tree('uccs', os.path.join(tmp, 'uccs'), 'uccs', ctx, bw, a))
        vgg_tree(os.path.join(tmp, 'vgg'), a.images, rng)
        a.host_rows = max(a.host_rows, 128)                      # a small image decodes in a millisecond or two
        res.update(run_tree('vgg', os.path.join(tmp, 'vgg'), 'vggface2', ctx, bw, a))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    rnd = lambda v: round(v, 4) if isinstance(v, float) else ([round(x, 4) for x in v] if isinstance(v, list) else v)
    print(json.dumps({k: rnd(v) for k, v in res.items()}))


if __name__ == '__main__':
    main()
