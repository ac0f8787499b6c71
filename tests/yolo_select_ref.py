"""NumPy restatement of fv_yolo_select_cands' contract (csrc/yolo_select.h), written from the definitions: per image the rows whose
capped arg-max class probability is > 0, in ascending order of it (equal scores by the smaller row), the first K of them, in
fv_decode_nms' layout.  Also the literal transcription of the reference's detect() tail over BoundBox objects that it is held
against on the CPU (face_detection.py:942-947 of the reference)."""
import numpy as np

INT_MAX = 2 ** 31 - 1


def select_ref(boxes, obj, cls, count, capacity, refuse_at, K, with_classes=True):
    """boxes (B, capacity, 4) int32, obj (B, capacity) float32, cls (B, capacity, nclass) float32, count (B,) int32 -> dict of
    boxes (B, K, 4) int32, cell (B, K) int32 (the row index), obj, score (B, K) float32, classes (B, K, nclass) float32 (None
    without with_classes), count (B,) int32.  Unused slots -1 / 0; a refused image (count >= refuse_at): count -1, no row read."""
    boxes, obj, cls, count = np.asarray(boxes), np.asarray(obj), np.asarray(cls), np.asarray(count)
    B, nclass = boxes.shape[0], cls.shape[2]
    assert boxes.shape == (B, capacity, 4) and obj.shape == (B, capacity) and cls.shape == (B, capacity, nclass) and count.shape == (B,)
    out = dict(boxes=np.full((B, K, 4), -1, np.int32), cell=np.full((B, K), -1, np.int32), obj=np.zeros((B, K), np.float32),
               score=np.zeros((B, K), np.float32), classes=np.zeros((B, K, nclass), np.float32) if with_classes else None,
               count=np.zeros(B, np.int32))
    for b in range(B):
        if int(count[b]) >= refuse_at:
            out['count'][b] = -1
            continue
        n = min(max(int(count[b]), 0), capacity)
        if n == 0:
            continue
        c = cls[b, :n]
        with np.errstate(invalid='ignore'):
            m = c[np.arange(n), np.argmax(c, axis=1)]                   # np.argmax: the first NaN wins -> m is NaN
            score = np.minimum(m, np.float32(1.0))                      # propagates the NaN
            # score > 0 on the bit pattern: sign clear, not zero, not a NaN -- a positive denormal counts whatever the float mode
            bits = score.view(np.uint32)
            keep = np.nonzero((bits > 0) & (bits <= 0x7F800000))[0]
        order = keep[np.argsort(bits[keep], kind='stable')][:K]         # positive floats order as their bit patterns
        k = len(order)
        out['boxes'][b, :k] = boxes[b, order]
        out['cell'][b, :k] = order
        out['obj'][b, :k] = obj[b, order]
        out['score'][b, :k] = score[order]
        if with_classes:
            out['classes'][b, :k] = c[order]
        out['count'][b] = k
    return out


def ties(out):
    """How many adjacent selected rows of one image share their score."""
    t = 0
    for b in range(len(out['count'])):
        k = max(int(out['count'][b]), 0)
        t += int((out['score'][b, 1:k] == out['score'][b, :k - 1]).sum()) if k > 1 else 0
    return t


class RefBoundBox(object):
    """The reference's BoundBox as far as detect()'s tail uses it (yolov3_detect.py:126-163)."""

    def __init__(self, xmin, ymin, xmax, ymax, objness=None, classes=None):
        self.xmin, self.ymin, self.xmax, self.ymax, self.objness, self.classes = xmin, ymin, xmax, ymax, objness, classes
        self.label = -1
        self.score = -1

    def get_label(self):
        if self.label == -1:
            self.label = np.argmax(self.classes)
        return self.label

    def get_score(self):
        if self.score == -1:
            self.score = self.classes[self.get_label()]
        return np.min([self.score, 1.0])


def reference_tail(boxes, obj, cls, n, K):
    """detect()'s tail, transcribed: BoundBox objects of the n decoded rows of one image, `get_score() > 0`, ascending stable
    argsort of the scores, the first K -> (list of kept BoundBox, their row indices)."""
    bbs = [RefBoundBox(boxes[r, 0], boxes[r, 1], boxes[r, 2], boxes[r, 3], objness=obj[r], classes=list(cls[r])) for r in range(n)]
    rows = [r for r in range(n) if bbs[r].get_score() > 0]
    scores = np.array([bbs[r].get_score() for r in rows])
    order = np.argsort(scores, kind='stable')[:K] if rows else []
    return [bbs[rows[i]] for i in order], [rows[i] for i in order]
