"""FaceIdentifier: facial IDs from the Darknet-53 base, trained with a triplet loss, and face identification against them.

Port of the reference's `src/space/face_identification.py` (fi.py): the model (fi.py:318-345), the facial-ID extractor
(`_make_fid_extractor`, fi.py:378-395), `train` (fi.py:616-643) over its two triplet sequences (fi.py:1490-1601 and the VGGFace2
variant), the facial-ID database (`make_facial_ids_db`, `register_facial_ids`, fi.py:645-770), `evaluate` (fi.py:772-992), `test`
(fi.py:994-1153) and `main` (fi.py:1715-1760) for the modes it dispatches, and the data mode (`create_db_fi` /
`save_extracted_face`, fi.py:78-280) that cuts the face crops and writes the subject db everything else reads.  The hot path is
the C ABI (fv_fid_extract, fv_fid_train_step(_dp), fv_adam_step, fv_letterbox_crops, fv_crop_nearest_u8, fv_gather_u8_f32,
fv_fid_match, fv_fid_pair_dists, fv_fid_mine_negatives, fv_fid_batch_train_step, fv_fid_cls_train_step, fv_draw_prims_u8); this
module holds the weights and drives it.
fi_conf.hps['triplet_mining'] ('semi_hard' / 'hardest'; not in the reference, off unless asked for) has
train() choose every triplet's negative from the model's current facial IDs;
fi_conf.hps['batch_mining'] ('batch_hard' / 'batch_semi_hard'; likewise opt-in) trains on batches of P subjects x K crops through
one tower and forms the triplets inside each batch.
fi_conf.hps['margin_softmax'] ('cosface' / 'arcface'; likewise opt-in) trains the same batches as a classification over the db's
subjects, a softmax with an additive margin over a class kernel of its own (fv_fid_cls_train_step).
fi_conf.hps['cluster'] (likewise opt-in) and the mode 'cluster' group the db's crops with subject_id -1 by DBSCAN over their facial
IDs on the device (fv_fid_cluster; cluster_unknown, register_clusters).
fi_conf.multi_gpu / num_gpus (the reference's keras.utils.multi_gpu_model around the triplet model,
fi.py:303-312, 348-361) trains data-parallel: main() starts num_gpus ranks, each runs fv_fid_train_step_dp on its contiguous slice
of every triplet batch and parallel.DataParallelTrainer all-reduces the gradients over RCCL while backward runs.
The reconstruction model (`create_face_reconst_model`, fi.py:1155-1488) is ReconModel over fv_recon_forward; the
reference never calls it from a mode, and neither does main().  evaluate() is a method only: main() does not dispatch
fi_conf.mode 'evaluate' yet.  Differences, documented in DESIGN.md: the BN moving-statistics update order
of the three towers (a -> p -> n), a zero gradient at a triplet distance of exactly 0, test() and evaluate() batching their
frames and crops (same rows), fp64 match distances, crops whose letterboxed side rounds to 0 being skipped (the reference's
cv.resize raises), the data mode's walk by source file (section 16), and evaluate() drawing its annotated frames on the device
with two documented departures from Pillow's rectangle (section 17)."""
import collections
import csv
import ctypes
import glob
import io
import json
import os
import pickle
import platform
import shutil
import time
from random import shuffle

import numpy as np
import torch

from . import weights
from ._lib import Context, FvError, lib, packed_args, ptr
from .annotate import MaskBlend, Outline, _font, annotation_prims, pack_masks      # noqa: F401 (part of this module's surface)
from .model import Model
from .weights import NUM_BASE_LAYERS

ALPHA = 0.2                     # fi.py:66
TRIPLET_MARGIN = ALPHA          # the loss's margin is the mining band's width: one number
BATCH_MINING_MODES = {'batch_hard': 0, 'batch_semi_hard': 1}   # fv_fid_batch_triplet_loss_grad's mode
BATCH_MAX_ROWS = 1024           # rows one fv_fid_batch_triplet_loss_grad call takes
MARGIN_SOFTMAX_KINDS = {'cosface': 0, 'arcface': 1}            # fv_fid_margin_softmax_loss_grad's kind
MARGIN_SOFTMAX_MARGINS = {'cosface': 0.35, 'arcface': 0.5}     # the papers' values (Wang et al. 2018; Deng et al. 2019)
MARGIN_SOFTMAX_SCALE = 30.0
CLASSES_MAX = 32768             # class rows one fv_fid_margin_softmax_loss_grad call takes
DENSE1_DIM = 64                 # the loss slices 0:64 / 64:128 / 128:192 (fi.py:72-76)
RESOURCE_TYPE_UCCS = 'uccs'
RESOURCE_TYPE_VGGFACE2 = 'vggface2'


def base_layers():
    from .engine import layer_table
    return layer_table()[:NUM_BASE_LAYERS]


def feature_size(image_size):
    """Flatten() length of the base output: (S/32)^2 * 1024 (173 056 at 416)."""
    return (int(image_size) // 32) ** 2 * 1024


def dense_offsets(image_size):
    """(kernel offset, bias offset) in the flat parameter vector: the dense kernel [F][64] follows the 52 base layers."""
    d = base_layers()[-1]
    k = d['beta_off'] + d['cout']
    return k, k + feature_size(image_size) * DENSE1_DIM


class FidModel(Model):
    """The device-side model: the flat parameter vector of fv_fid_param_count (base layers at their fv_layer offsets, then the
    dense kernel and bias), the BN moving statistics (fv_state_count), the Adam state, and the calls into the library."""

    BN_UPDATES_PER_STEP = 3         # one per tower

    def __init__(self, image_size, device=0):
        self.image_size = int(image_size)
        n_params = int(lib().fv_fid_param_count(self.image_size))
        if n_params <= 0:
            raise ValueError('image_size must be a positive multiple of 32')
        super(FidModel, self).__init__(Context(device), base_layers(), n_params, lib().fv_state_count())
        self.F = feature_size(self.image_size)
        self.kernel_off, self.bias_off = dense_offsets(self.image_size)
        self.bn_zero_debias = True      # Keras 2.2.4's zero-debiased BN update (Engine.bn_zero_debias)

    # ------------------------------------------------------------------ parameters
    def init_dense(self, seed=0):
        """Keras defaults of Dense(64) (fi.py:327): glorot_uniform kernel, limit sqrt(6 / (F + 64)), zero bias."""
        g = torch.Generator().manual_seed(seed)
        lim = float(np.sqrt(6.0 / (self.F + DENSE1_DIM)))
        n = self.F * DENSE1_DIM
        self.params[self.kernel_off:self.kernel_off + n] = ((torch.rand(n, generator=g) * 2 - 1) * lim).to(self.dev)
        self.params[self.bias_off:self.bias_off + DENSE1_DIM] = 0

    def dense_kernel(self):
        return self.params[self.kernel_off:self.bias_off].view(self.F, DENSE1_DIM)

    def dense_bias(self):
        return self.params[self.bias_off:self.bias_off + DENSE1_DIM]

    def _workspace_bytes(self, batch, image_size, training):
        return lib().fv_fid_workspace_bytes(batch, image_size, training)

    def _as_input(self, x):
        if isinstance(x, np.ndarray) and x.dtype == np.uint8:
            x = x.astype(np.float32) / np.float32(255.0)
        x = torch.as_tensor(x)
        if x.dtype == torch.uint8:
            x = x.to(torch.float32) / 255.0
        if x.dtype != torch.float32 or x.device != self.dev:
            x = x.to(device=self.dev, dtype=torch.float32)
        x = x.contiguous()
        if x.dim() != 4 or x.shape[1] != self.image_size or x.shape[2] != self.image_size or x.shape[3] != 3:
            raise ValueError('expected images of shape (B, %d, %d, 3), got %r' % (self.image_size, self.image_size, tuple(x.shape)))
        return x

    # ------------------------------------------------------------------ extraction (fi.py:378-395)
    def extract_device(self, x):
        """x (B,S,S,3) in [0,1] (uint8 crops are divided by 255, fi.py:1577) -> (B,64) facial IDs, float32 CUDA tensor."""
        return self._in_parts(self._extract, self._as_input(x))

    def _extract(self, x):
        B = x.shape[0]
        ws = self._workspace(B, self.image_size, False)
        fid = torch.empty((B, DENSE1_DIM), dtype=torch.float32, device=self.dev)
        rc = lib().fv_fid_extract(self.ctx.handle, ptr(self.params), ptr(self.state), ptr(x), B, self.image_size, ptr(ws), ws.numel(),
                                  ptr(fid))
        self.ctx.check(rc, 'fv_fid_extract')
        return fid

    # ------------------------------------------------------------------ training
    def forward_backward(self, xa, xp, xn, on_bucket=None, loss_weight=1.0):
        """Triplet forward + loss + backward (fv_fid_train_step_dp): gradients in self.grads, BN moving statistics updated
        a -> p -> n; returns the loss as a 1-element CUDA tensor (no host sync).  on_bucket(offset, count) is called as gradient
        ranges complete (descending offsets: the dense bias and kernel first, then the base layers from the third tower's pass),
        the protocol of Engine.forward_backward -- parallel.DataParallelTrainer drives either.  loss_weight: this slice's share
        n_r / N of a merged data-parallel batch: scales the gradients, not the loss."""
        self.ensure_optimizer()
        xa, xp, xn = self._as_input(xa), self._as_input(xp), self._as_input(xn)
        B = xa.shape[0]
        if xp.shape != xa.shape or xn.shape != xa.shape:
            raise ValueError('anchor, positive and negative batches differ in shape')
        ws = self._workspace(B, self.image_size, True)
        cb, errors = self._bucket_fn(on_bucket)
        return self._train_call('fv_fid_train_step_dp', ptr(xa), ptr(xp), ptr(xn), B, self.image_size, ptr(ws), ws.numel(),
                                ptr(self.grads), ptr(self._loss), float(loss_weight), cb, None, errors=errors)

    def train_on_batch(self, xa, xp, xn, lr, beta_1, beta_2, decay=0.0):
        loss = self.forward_backward(xa, xp, xn)
        self.adam_step(lr, beta_1, beta_2, decay)
        return loss

    # ------------------------------------------------------------------ training on a labelled batch
    def _grown_workspace(self, name, n, what, shape):
        """The workspace of a one-tower step, under a key of its own: the triplet step's and extraction's stay.  One buffer of n
        bytes, grown to the largest call so far (a PK batch is short where a subject has fewer than K crops)."""
        if n == 0:
            raise FvError('unsupported %s %r' % (what, shape))
        key = (0, self.image_size, name)
        if key not in self._ws or self._ws[key].numel() < n:
            self._ws.pop(key, None)
            self._ws[key] = torch.empty(int(n), dtype=torch.uint8, device=self.dev)
        return self._ws[key]

    def _batch_workspace(self, M):
        """The workspace of fv_fid_batch_train_step."""
        return self._grown_workspace('labelled_batch', lib().fv_fid_batch_workspace_bytes(M, self.image_size), 'batch/image_size',
                                     (M, self.image_size))

    def _row_ints(self, who, what, values, M):
        """values (a subject or a label per image of the batch) -> (M,) int32 on the device; a batch is at most BATCH_MAX_ROWS."""
        rows = torch.as_tensor(values if torch.is_tensor(values) else np.asarray(values)).to(device=self.dev, dtype=torch.int32).contiguous()
        if rows.dim() != 1 or rows.shape[0] != M:
            raise ValueError('%s expects one %s per image (%d images, %ss of shape %r)' % (who, what, M, what, tuple(rows.shape)))
        if M > BATCH_MAX_ROWS:
            raise ValueError('%s takes at most %d images, got %d' % (who, BATCH_MAX_ROWS, M))
        return rows

    def forward_backward_batch(self, x, subjects, mode='batch_hard', margin=None):
        """One tower over the labelled batch x (M,S,S,3), subjects (M,) int32 (< 0: an unknown identity), triplets mined inside
        the batch (fv_fid_batch_train_step; mode 'batch_hard' / 'batch_semi_hard' or 0 / 1; margin: TRIPLET_MARGIN): gradients
        in self.grads, ONE update of the BN moving statistics; returns the loss as a 1-element CUDA tensor (no host sync).
        self.batch_selection keeps pos_index, neg_index, kind (int32), d_ap, d_an (float64), CUDA tensors of M."""
        self.ensure_optimizer()
        x = self._as_input(x)
        M = x.shape[0]
        sub = self._row_ints('forward_backward_batch', 'subject', subjects, M)
        code = BATCH_MINING_MODES.get(mode, mode)
        if isinstance(code, bool) or code not in (0, 1):
            raise ValueError('forward_backward_batch: mode %r (available: %s)' % (mode, ', '.join(sorted(BATCH_MINING_MODES))))
        ws = self._batch_workspace(M)
        sel = dict(pos_index=torch.empty(M, dtype=torch.int32, device=self.dev), neg_index=torch.empty(M, dtype=torch.int32, device=self.dev),
                   kind=torch.empty(M, dtype=torch.int32, device=self.dev), d_ap=torch.empty(M, dtype=torch.float64, device=self.dev),
                   d_an=torch.empty(M, dtype=torch.float64, device=self.dev))
        loss = self._train_call('fv_fid_batch_train_step', ptr(x), ptr(sub), M, self.image_size, int(code),
                                float(TRIPLET_MARGIN if margin is None else margin), ptr(ws), ws.numel(), ptr(self.grads), ptr(self._loss),
                                ptr(sel['pos_index']), ptr(sel['neg_index']), ptr(sel['kind']), ptr(sel['d_ap']), ptr(sel['d_an']),
                                bn_updates=1)
        self.batch_selection = sel
        return loss

    def train_on_labelled_batch(self, x, subjects, mode, lr, beta_1, beta_2, decay=0.0, margin=None):
        loss = self.forward_backward_batch(x, subjects, mode, margin)
        self.adam_step(lr, beta_1, beta_2, decay)
        return loss

    # ------------------------------------------------------------------ training with a margin softmax
    def init_classes(self, C, seed=0):
        """The class kernel [C][64] of the margin softmax: rows drawn from np.random.RandomState(seed).standard_normal, each
        normalised to length 1, float32; its gradient and Adam vectors start at zero."""
        C = int(C)
        if not 1 <= C <= CLASSES_MAX:
            raise ValueError('init_classes takes 1 .. %d classes, got %d' % (CLASSES_MAX, C))
        w = np.random.RandomState(int(seed)).standard_normal((C, DENSE1_DIM))
        w = (w / np.sqrt((w * w).sum(-1, keepdims=True))).astype(np.float32)
        self.set_classes(w)

    def set_classes(self, kernel):
        self.class_kernel = torch.as_tensor(np.asarray(kernel, np.float32)).to(self.dev).contiguous()
        self.class_grads = torch.zeros_like(self.class_kernel)
        self.class_m = torch.zeros_like(self.class_kernel)
        self.class_v = torch.zeros_like(self.class_kernel)

    def _cls_workspace(self, M):
        """The workspace of fv_fid_cls_train_step."""
        C = int(self.class_kernel.shape[0])
        return self._grown_workspace('classified_batch', lib().fv_fid_cls_workspace_bytes(M, C, self.image_size),
                                     'batch/classes/image_size', (M, C, self.image_size))

    def forward_backward_classes(self, x, labels, kind='cosface', scale=MARGIN_SOFTMAX_SCALE, margin=None):
        """One tower over the labelled batch x (M,S,S,3), labels (M,) int32 class indices (< 0: an unknown identity), the margin
        softmax over self.class_kernel (fv_fid_cls_train_step; kind 'cosface' / 'arcface' or 0 / 1; margin: the paper's):
        gradients in self.grads and self.class_grads, ONE update of the BN moving statistics; returns the loss as a 1-element
        CUDA tensor (no host sync).  self.class_selection keeps pred (int32) and cos_t (float64), CUDA tensors of M.  Labels
        handed over as a host array are checked against the class count."""
        if getattr(self, 'class_kernel', None) is None:
            raise ValueError('forward_backward_classes needs a class kernel: call init_classes first')
        self.ensure_optimizer()
        x = self._as_input(x)
        M, C = x.shape[0], int(self.class_kernel.shape[0])
        if not torch.is_tensor(labels):
            labels = np.asarray(labels)
            if labels.size and int(labels.max()) >= C:
                raise ValueError('forward_backward_classes: label %d is not below the %d classes' % (int(labels.max()), C))
        lab = self._row_ints('forward_backward_classes', 'label', labels, M)
        name = kind if isinstance(kind, str) else {v: k for k, v in MARGIN_SOFTMAX_KINDS.items()}.get(kind)
        if isinstance(kind, bool) or name not in MARGIN_SOFTMAX_KINDS:
            raise ValueError('forward_backward_classes: kind %r (available: %s)' % (kind, ', '.join(sorted(MARGIN_SOFTMAX_KINDS))))
        margin = MARGIN_SOFTMAX_MARGINS[name] if margin is None else margin
        ws = self._cls_workspace(M)
        sel = dict(pred=torch.empty(M, dtype=torch.int32, device=self.dev), cos_t=torch.empty(M, dtype=torch.float64, device=self.dev))
        loss = self._train_call('fv_fid_cls_train_step', ptr(x), ptr(lab), M, self.image_size, ptr(self.class_kernel), C,
                                MARGIN_SOFTMAX_KINDS[name], float(scale), float(margin), ptr(ws), ws.numel(), ptr(self.grads),
                                ptr(self.class_grads), ptr(self._loss), ptr(sel['pred']), ptr(sel['cos_t']), bn_updates=1)
        self.class_selection = sel
        return loss

    def train_on_classified_batch(self, x, labels, kind, scale, margin, lr, beta_1, beta_2, decay=0.0):
        """forward_backward_classes, then Adam over the class kernel (its own m / v; the same iteration, lr, betas and decay)
        and over the model."""
        from . import ops
        loss = self.forward_backward_classes(x, labels, kind, scale, margin)
        ops.adam_step(self.ctx, self.class_kernel, self.class_grads, self.class_m, self.class_v, self.iterations, lr, beta_1, beta_2,
                      1e-7, decay)
        self.adam_step(lr, beta_1, beta_2, decay)
        return loss

    # ------------------------------------------------------------------ checkpoint (fi.py:643 model.save, fi.py:304 load_model)
    def save(self, path):
        """face_identifier.h5 in Keras' weight layout: the base as the nested model 'base', then dense1/kernel:0 [F][64] and
        dense1/bias:0; this build's Adam state and step counts under /fv."""
        dense = [('dense1/kernel:0', self.dense_kernel().cpu().numpy()), ('dense1/bias:0', self.dense_bias().cpu().numpy())]
        self._save_h5(path, 'base', {'dense1': dense}, bn_updates=np.int64(self.bn_updates))

    def load(self, path):
        fv = self._load(path, read_more=self._read_dense)
        self.bn_updates = int(fv.get('bn_updates', 0))

    def _read_dense(self, path, datasets, p):
        kern = [k for k in datasets if k.endswith('/dense1/kernel:0')]
        bias = [k for k in datasets if k.endswith('/dense1/bias:0')]
        if len(kern) != 1 or len(bias) != 1:
            raise FvError('%s holds no dense1 layer' % path)
        K = np.asarray(datasets[kern[0]], np.float32)
        b = np.asarray(datasets[bias[0]], np.float32)
        if K.shape != (self.F, DENSE1_DIM) or b.shape != (DENSE1_DIM,):
            raise FvError('%s: dense1 has shapes %r / %r, this model expects (%d, %d) / (%d,)'
                          % (path, K.shape, b.shape, self.F, DENSE1_DIM, DENSE1_DIM))
        p[self.kernel_off:self.bias_off] = K.reshape(-1)
        p[self.bias_off:self.bias_off + DENSE1_DIM] = b


class FidExtractor(object):
    """fid_extractor (fi.py:378-395): base -> flatten -> dense1 -> l2_norm with inference-mode BN; `predict` as Keras (numpy)."""

    def __init__(self, model):
        self.model = model

    def predict_device(self, images):
        return self.model.extract_device(images)

    def predict(self, images):
        return self.predict_device(images).cpu().numpy()


# ----------------------------------------------------------------------------- reconstruction model (fi.py:1155-1488)
RECON_MODEL_PATH = 'face_vijnana_recon.h5'
_BN_WEIGHTS = ('gamma', 'beta', 'moving_mean', 'moving_variance')


def recon_offsets(image_size):
    """The fv_recon_param_count layout: dict(dense, bias, bn, count) in floats -- the 52 conv kernels at their fv_layer w_off,
    the dense kernel [F][64], the bias [F], then per layer gamma, beta, moving mean, moving variance ([4][cout]); layer l's four
    vectors begin at bn + 4 * (mean_off / 2)."""
    d = base_layers()[-1]
    F = feature_size(image_size)
    dense = d['beta_off'] + d['cout']
    bias = dense + F * DENSE1_DIM
    bn = bias + F
    return dict(dense=dense, bias=bias, bn=bn, count=bn + 4 * (d['var_off'] + d['cout']) // 2)


def recon_stage_order():
    """Indices into the layer table in the order the model runs its stages (fi.py:1187-1484): 51 .. 0."""
    return list(range(NUM_BASE_LAYERS - 1, -1, -1))


def recon_h5_layout(image_size):
    """[(dataset path, shape)] of face_vijnana_recon.h5, Keras' weight layout under the reference's layer names: dense1 (the
    TRANSPOSED dense kernel [64][F] and a bias [F], fi.py:1179-1180), then per stage its BatchNormalization `bnorm_<i>` and its
    Conv2DTranspose, named as the conv layer it mirrors (`conv_<i>`, i the Darknet index; `output` for layer 0, fi.py:1475) with
    that layer's (k, k, Cin, Cout) kernel.  Needs no device."""
    F = feature_size(image_size)
    out = [('/model_weights/dense1/dense1/kernel:0', (DENSE1_DIM, F)), ('/model_weights/dense1/dense1/bias:0', (F,))]
    layers = base_layers()
    for l in recon_stage_order():
        d = layers[l]
        i = d['darknet_index']
        out += [('/model_weights/bnorm_%d/bnorm_%d/%s:0' % (i, i, w), (d['cout'],)) for w in _BN_WEIGHTS]
        name = 'output' if l == 0 else 'conv_%d' % i
        out.append(('/model_weights/%s/%s/kernel:0' % (name, name), (d['ksize'], d['ksize'], d['cin'], d['cout'])))
    return out


class ReconModel(Model):
    """recon_model of create_face_reconst_model (fi.py:1155-1488): a facial ID (64 floats) back through the transposed dense1
    layer and the 52 base layers as Conv2DTranspose layers to an (S, S, 3) image -- fv_recon_forward; the arithmetic is stated in
    include/fv_hotpath.h.  The flat parameter vector is fv_recon_param_count's (recon_offsets); there is no BN-state vector: every
    stage's BatchNormalization is a layer of this model and its four vectors are parameters."""

    def __init__(self, image_size, device=0, ctx=None):
        self.image_size = int(image_size)
        n_params = int(lib().fv_recon_param_count(self.image_size))
        if n_params <= 0:
            raise ValueError('image_size must be a positive multiple of 32')
        super(ReconModel, self).__init__(ctx if ctx is not None else Context(device), base_layers(), n_params, 0)
        self.F = feature_size(self.image_size)
        self.off = recon_offsets(self.image_size)
        assert self.off['count'] == n_params
        self.fresh_bn()

    # ------------------------------------------------------------------ parameters
    def bn_slice(self, l, which):
        """Range of vector `which` (0 gamma, 1 beta, 2 moving mean, 3 moving variance) of layer l's BatchNormalization."""
        d = self.layers[l]
        a = self.off['bn'] + 4 * (d['mean_off'] // 2) + which * d['cout']
        return slice(a, a + d['cout'])

    def kernel_slice(self, l):
        d = self.layers[l]
        return slice(d['w_off'], d['w_off'] + d['cout'] * d['ksize'] * d['ksize'] * d['cin'])

    def dense_kernel(self):
        """[F][64]: dense1's kernel as the FaceIdentifier holds it (the model multiplies by its transpose)."""
        return self.params[self.off['dense']:self.off['bias']].view(self.F, DENSE1_DIM)

    def dense_bias(self):
        return self.params[self.off['bias']:self.off['bn']]

    def fresh_bn(self):
        """BatchNormalization.from_config (fi.py:1197): a new layer -- gamma 1, beta 0, moving mean 0, moving variance 1."""
        for l in range(len(self.layers)):
            self.params[self.bn_slice(l, 0)] = 1.0
            self.params[self.bn_slice(l, 1)] = 0.0
            self.params[self.bn_slice(l, 2)] = 0.0
            self.params[self.bn_slice(l, 3)] = 1.0

    @classmethod
    def from_identifier(cls, fid_model, seed=None):
        """The snapshot create_face_reconst_model takes (set_weights copies): the 52 conv kernels and the dense kernel of
        fid_model, a bias drawn as np.random.RandomState(seed).rand(F) (the reference: np.random.rand, fi.py:1180), fresh BN.
        Training fid_model afterwards does not change this model."""
        m = cls(fid_model.image_size, ctx=fid_model.ctx)
        for l in range(len(m.layers)):
            m.params[m.kernel_slice(l)] = fid_model.params[m.kernel_slice(l)]
        m.dense_kernel().copy_(fid_model.dense_kernel())
        bias = np.random.RandomState(seed).rand(m.F).astype(np.float32)
        m.dense_bias().copy_(torch.from_numpy(bias))
        return m

    # ------------------------------------------------------------------ inference
    def _workspace_bytes(self, batch, image_size, training):
        return lib().fv_recon_workspace_bytes(batch, image_size)

    def _as_ids(self, ids):
        ids = torch.as_tensor(ids)
        if ids.dtype != torch.float32 or ids.device != self.dev:
            ids = ids.to(device=self.dev, dtype=torch.float32)
        ids = ids.contiguous()
        if ids.dim() != 2 or ids.shape[1] != DENSE1_DIM:
            raise ValueError('expected facial IDs of shape (N, %d), got %r' % (DENSE1_DIM, tuple(ids.shape)))
        return ids

    def predict_device(self, ids):
        """ids (N,64) -> (N,S,S,3) float32 CUDA tensor (no activation on the output, fi.py:1483)."""
        return self._in_parts(self._forward, self._as_ids(ids), image_size=self.image_size)

    def predict(self, ids):
        return self.predict_device(ids).cpu().numpy()

    def _forward(self, ids):
        N, S = ids.shape[0], self.image_size
        ws = self._workspace(N, S, False)
        out = torch.empty((N, S, S, 3), dtype=torch.float32, device=self.dev)
        rc = lib().fv_recon_forward(self.ctx.handle, ptr(self.params), ptr(ids), N, S, ptr(ws), ws.numel(), ptr(out))
        self.ctx.check(rc, 'fv_recon_forward')
        return out

    # ------------------------------------------------------------------ checkpoint (fi.py:1488 recon_model.save, fi.py:1161 load_model)
    def _tensors(self):
        """{dataset path: array} in the recon_h5_layout order."""
        p = self.params.cpu().numpy()
        out = collections.OrderedDict()
        for name, shape in recon_h5_layout(self.image_size):
            layer, weight = name.split('/')[-2], name.split('/')[-1][:-2]
            if layer == 'dense1':
                a = p[self.off['dense']:self.off['bias']].reshape(self.F, DENSE1_DIM).T if weight == 'kernel' else p[self.off['bias']:self.off['bn']]
            else:
                l = self._layer_of(layer)
                if weight == 'kernel':
                    d = self.layers[l]
                    a = p[self.kernel_slice(l)].reshape(d['cout'], d['ksize'], d['ksize'], d['cin']).transpose(1, 2, 3, 0)   # OHWI -> HWIO
                else:
                    a = p[self.bn_slice(l, _BN_WEIGHTS.index(weight))]
            out[name] = np.ascontiguousarray(a, dtype=np.float32)
            assert out[name].shape == tuple(shape), name
        return out

    def _layer_of(self, name):
        if name == 'output':
            return 0
        i = int(name.split('_')[1])
        return [l for l, d in enumerate(self.layers) if d['darknet_index'] == i][0]

    def save(self, path):
        """face_vijnana_recon.h5 in Keras' weight layout (recon_h5_layout) through hdf5_lite: readable by h5py and by
        `load_weights` of a model built as the reference builds it; it holds no model_config, so not by `load_model`."""
        from .hdf5_lite import write_hdf5
        data = self._tensors()
        groups = collections.OrderedDict()
        for name in data:
            groups.setdefault(name.split('/')[2], []).append('/'.join(name.split('/')[3:]))
        fixed = lambda xs: np.array([x.encode('utf8') for x in xs])
        attrs = {'/': {'keras_version': b'2.2.4', 'backend': b'tensorflow'},
                 '/model_weights': {'layer_names': fixed(list(groups)), 'backend': b'tensorflow', 'keras_version': b'2.2.4'}}
        for g, names in groups.items():
            attrs['/model_weights/' + g] = {'weight_names': fixed(names)}
        write_hdf5(path, data, attrs)

    def load(self, path):
        """A file written by save() (any HDF5 file with these datasets under these names).  Everything is checked before
        anything is changed."""
        from .hdf5_lite import read_hdf5
        datasets, _ = read_hdf5(path)
        p = np.zeros(self.n_params, np.float32)
        for name, shape in recon_h5_layout(self.image_size):
            if name not in datasets:
                raise FvError('%s lacks %s' % (path, name))
            a = np.asarray(datasets[name], np.float32)
            if a.shape != tuple(shape):
                raise FvError('%s: %s has shape %r, this model expects %r' % (path, name, a.shape, tuple(shape)))
            layer, weight = name.split('/')[-2], name.split('/')[-1][:-2]
            if layer == 'dense1':
                if weight == 'kernel':
                    p[self.off['dense']:self.off['bias']] = a.T.reshape(-1)
                else:
                    p[self.off['bias']:self.off['bn']] = a
            else:
                l = self._layer_of(layer)
                if weight == 'kernel':
                    p[self.kernel_slice(l)] = a.transpose(3, 0, 1, 2).reshape(-1)          # HWIO -> OHWI
                else:
                    p[self.bn_slice(l, _BN_WEIGHTS.index(weight))] = a
        self.params.copy_(torch.from_numpy(p))


# ----------------------------------------------------------------------------- triplet sequences (fi.py:1490-1601)
def make_triplets(db, rng=None):
    """The reference's triplet list: for every subject (in sorted subject_id order) and every pair k < l of its images, the triplet
    (k, l, a random image of another subject), as row labels of `db`.  rng: numpy RandomState (np.random by default)."""
    rng = np.random if rng is None else rng
    t_indexes = np.asarray(db.index)
    triplets = []
    for _sid, df in db.groupby('subject_id'):
        own = np.asarray(df.index)
        others = t_indexes[~np.isin(t_indexes, own)]
        for k in range(0, own.shape[0] - 1):
            for l in range(k + 1, own.shape[0]):
                triplets.append((own[k], own[l], rng.choice(others, size=1)[0]))
    return triplets


def num_batches(n, batch_size):
    """hps['step'] as the sequences set it: whole batches plus one short last batch."""
    return n // batch_size + (1 if n % batch_size else 0)


def _imread(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert('RGB'))


class _TripletSequence(object):
    DB_FILE = None
    PICKLE_FILE = None
    FACES_DIR = None

    def __init__(self, raw_data_path, hps, nn_arch, load_flag=True):
        import pandas as pd
        self.raw_data_path = raw_data_path
        self.hps = hps
        self.nn_arch = nn_arch
        self.db = pd.read_csv(self.DB_FILE).iloc[:, 1:]
        if load_flag:
            with open(self.PICKLE_FILE, 'rb') as f:
                self.img_triplet_pairs = pickle.load(f)
        else:
            self.img_triplet_pairs = make_triplets(self.db)
            shuffle(self.img_triplet_pairs)
            with open(self.PICKLE_FILE, 'wb') as f:
                pickle.dump(self.img_triplet_pairs, f)
        self.batch_size = int(self.hps['batch_size'])
        self.hps['step'] = num_batches(len(self.img_triplet_pairs), self.batch_size)

    def __len__(self):
        return self.hps['step']

    def path(self, label):
        """The crop file of db row `label`."""
        return os.path.join(self.raw_data_path, self.FACES_DIR, self.db.loc[label, 'face_file'])

    def _image(self, label):
        img = _imread(self.path(label))
        return img.astype(np.float32) / np.float32(255.0)

    def rows(self, index):
        """The triplets of batch `index` (the last batch is the short one)."""
        end = len(self.img_triplet_pairs) if index == self.hps['step'] - 1 else (index + 1) * self.batch_size
        return self.img_triplet_pairs[index * self.batch_size:end]

    def __getitem__(self, index):
        return self.load(self.rows(index))

    def load(self, rows):
        """The Keras batch of the triplets `rows`: only their images are read."""
        xa = np.asarray([self._image(t[0]) for t in rows])
        xp = np.asarray([self._image(t[1]) for t in rows])
        xn = np.asarray([self._image(t[2]) for t in rows])
        return {'input_a': xa, 'input_p': xp, 'input_n': xn}, {'output': np.zeros((len(rows), 3 * DENSE1_DIM))}


class TrainingSequence(_TripletSequence):
    """UCCS crops: subject_image_db.csv, <raw_data_path>/subject_faces/, img_triplet_pairs.pickle (fi.py:1490-1601)."""
    DB_FILE = 'subject_image_db.csv'
    PICKLE_FILE = 'img_triplet_pairs.pickle'
    FACES_DIR = 'subject_faces'


class TrainingSequenceVGGFace2(_TripletSequence):
    """VGGFace2 crops: subject_image_vggface2_db.csv, <raw_data_path>/subject_faces_vggface2/, img_triplet_pairs_vggface2.pickle."""
    DB_FILE = 'subject_image_vggface2_db.csv'
    PICKLE_FILE = 'img_triplet_pairs_vggface2.pickle'
    FACES_DIR = 'subject_faces_vggface2'


def slice_triplets(rows, world_size, rank):
    """This rank's part of a triplet batch, as keras.utils.multi_gpu_model cuts the three inputs (parallel.slice_batch:
    contiguous, the remainder to the last rank) -> (rows of the slice, its weight n_r / n in the merged-batch mean), or None on
    EVERY rank when the batch holds fewer triplets than there are ranks."""
    from .parallel import slice_batch
    sl = slice_batch(len(rows), world_size, rank)
    if sl is None:
        return None
    return rows[sl[0]:sl[1]], sl[2]


# ----------------------------------------------------------------------------- identification helpers (fi.py:645-770, 994-1153)
MAX_ROWS_PER_IMAGE = 60          # test() writes at most 60 rows per image (fi.py:1057-1058)


def db_files(resource_type):
    """(subject db csv, faces directory, facial-ID h5, registry pickle) of a resource type (fi.py:647-700, 702-770)."""
    if resource_type == RESOURCE_TYPE_UCCS:
        return 'subject_image_db.csv', 'subject_faces', 'subject_facial_ids.h5', 'ref_facial_id_db.pickle'
    if resource_type == RESOURCE_TYPE_VGGFACE2:
        return ('subject_image_vggface2_db.csv', 'subject_faces_vggface2', 'subject_facial_vggface2_ids.h5',
                'ref_facial_id_vggface2_db.pickle')
    raise ValueError('resource type is not valid.')


def lb_side_ok(h, w, image_size):
    """False when the letterboxed crop's short side rounds to 0 (int(h / w * S) as fi.py:1071-1093 computes it): cv.resize
    would reject it; fv_letterbox_crops does."""
    S = int(image_size)
    return (int(h / w * S) if w >= h else int(w / h * S)) >= 1


def crop_rect(box, h, w):
    """The face crop of test() (fi.py:1061-1063): `image_o[(t - 1):(b - 1), (l - 1):(r - 1)]` with l, t, r, b = int() of the
    projected box, Python slice semantics on an h x w image (a start of -1 -- a box on the top or left edge -- counts from the end
    and leaves the crop empty).  -> (y0, x0, rows, cols), or None for an empty crop (the reference skips it, fi.py:1072-1073)."""
    l, t, r, b = int(box.xmin), int(box.ymin), int(box.xmax), int(box.ymax)
    return slice_rect(t - 1, b - 1, l - 1, r - 1, h, w)


def slice_rect(y0, y1, x0, x1, h, w):
    """`image[y0:y1, x0:x1]` of an h x w image with Python slice semantics -> (y0, x0, rows, cols), or None when it is empty."""
    ys = range(*slice(y0, y1).indices(int(h)))
    xs = range(*slice(x0, x1).indices(int(w)))
    if len(ys) == 0 or len(xs) == 0:
        return None
    return ys.start, xs.start, len(ys), len(xs)


def crop_rects(boxes, h, w, image_size):
    """crop_rect of every box, None also where the letterboxed side would round to 0 (a deviation: the reference's cv.resize
    raises there)."""
    out = []
    for box in boxes:
        c = crop_rect(box, h, w)
        out.append(c if c is not None and lb_side_ok(c[2], c[3], image_size) else None)
    return out


def matched_boxes(rects, best_dist, sim_th, limit=MAX_ROWS_PER_IMAGE):
    """Indices of the boxes of one image that test() / evaluate() write a row for (fi.py:1057-1148, 864-941): boxes in detector
    order, those without a crop skipped, a match farther than sim_th skipped, at most `limit` rows."""
    out = []
    for k, rect in enumerate(rects):
        if len(out) >= limit:
            break
        if rect is None or best_dist[k] > sim_th:
            continue
        out.append(k)
    return out


def identification_rows(file_name, boxes, rects, best_index, best_dist, subject_ids, sim_th, limit=MAX_ROWS_PER_IMAGE):
    """The rows test() writes for one image (fi.py:1057-1148): boxes in detector order, those without a crop skipped, a match
    farther than sim_th skipped, at most `limit` rows written.  best_index / best_dist: per box (read only where a row can still be
    written).  -> csv text, `str()` of each value exactly as fi.py:1143-1148."""
    base = file_name.split('\\')[-1] if platform.system() == 'Windows' else file_name.split('/')[-1]
    out = []
    for k in matched_boxes(rects, best_dist, sim_th, limit):
        box = boxes[k]
        subject_id = subject_ids[int(best_index[k])]
        out.append(base + ',' + str(subject_id) + ',' + str(box.xmin) + ',' + str(box.ymin) + ',')
        out.append(str(box.xmax - box.xmin) + ',' + str(box.ymax - box.ymin) + ',' + str(box.get_score()) + '\n')
    return ''.join(out)


def subject_mean(facial_ids):
    """A subject's registered facial ID exactly as register_facial_ids computes it (fi.py:727): the pandas column mean."""
    import pandas as pd
    return np.asarray(pd.DataFrame(facial_ids).mean())


def write_facial_ids_h5(path, names, facial_ids, subject_ids):
    """subject_facial_ids.h5 (fi.py:650-668): one root dataset per face file (float32 (64,)) with attribute subject_id."""
    from .hdf5_lite import write_hdf5
    datasets, attrs = {}, {}
    for name, fid, sid in zip(names, facial_ids, subject_ids):
        datasets['/' + name] = np.asarray(fid, np.float32)
        attrs['/' + name] = {'subject_id': np.int64(sid)}
    write_hdf5(path, datasets, attrs)


def read_facial_ids_h5(path):
    """-> {face file: (facial ID, subject_id)} of write_facial_ids_h5's file."""
    from .hdf5_lite import read_hdf5
    data, attrs = read_hdf5(path)
    return {k[1:]: (np.asarray(v), int(np.asarray(attrs[k]['subject_id']).reshape(-1)[0])) for k, v in data.items()}


def fid_match(ctx, queries, registry):
    """fv_fid_match: queries (n, 64), registry (m, 64) float32 CUDA tensors -> (best index int32, best distance float64) CUDA
    tensors of n (stream-ordered)."""
    q = queries.contiguous()
    r = registry.contiguous()
    n, m = int(q.shape[0]), int(r.shape[0])
    idx = torch.empty(n, dtype=torch.int32, device=q.device)
    dist = torch.empty(n, dtype=torch.float64, device=q.device)
    if n == 0:
        return idx, dist
    if q.dtype != torch.float32 or r.dtype != torch.float32 or q.shape[1:] != (DENSE1_DIM,) or r.shape[1:] != (DENSE1_DIM,):
        raise ValueError('fid_match expects float32 (n, 64) queries and (m, 64) registry')
    ctx.check(lib().fv_fid_match(ctx.handle, ptr(q), n, ptr(r), m, ptr(idx), ptr(dist)), 'fv_fid_match')
    return idx, dist


# ----------------------------------------------------------------------------- clustering of facial IDs
CLUSTER_MAX_ROWS = 65536         # FV_FID_CLUSTER_MAX_N of csrc/fid_cluster.h
CLUSTER_MIN_PTS = 3
CLUSTER_KEYS = ('eps', 'min_pts', 'register')


def fid_cluster(ctx, ids, eps, min_pts, workspace=None):
    """fv_fid_cluster: DBSCAN over ids (n, 64) float32 CUDA tensor under fid_match's distance -> dict of CUDA tensors: labels, via,
    n_nbr (n,) int32, core (n,) uint8, n_clusters (1,) int32 (csrc/fid_cluster.h defines them).  Stream-ordered, no copy back.
    workspace: a CUDA tensor of at least fv_fid_cluster_workspace_bytes(n) bytes (its contents are ignored); None: one kept on the
    context and grown to the largest call so far."""
    if ids.dtype != torch.float32 or ids.dim() != 2 or ids.shape[1] != DENSE1_DIM:
        raise ValueError('fid_cluster expects float32 (n, 64) ids')
    x = ids.contiguous()
    n, dev = int(x.shape[0]), x.device
    out = dict(labels=torch.empty(n, dtype=torch.int32, device=dev), via=torch.empty(n, dtype=torch.int32, device=dev),
               n_nbr=torch.empty(n, dtype=torch.int32, device=dev), core=torch.empty(n, dtype=torch.uint8, device=dev),
               n_clusters=torch.zeros(1, dtype=torch.int32, device=dev))
    if n == 0:
        return out
    need = int(lib().fv_fid_cluster_workspace_bytes(n))
    if need == 0:
        raise ValueError('fid_cluster takes 1..%d rows, got %d' % (CLUSTER_MAX_ROWS, n))
    if workspace is None:
        workspace = getattr(ctx, '_fid_cluster_ws', None)
        if workspace is None or workspace.numel() < need or workspace.device != dev:
            ctx._fid_cluster_ws = None
            workspace = ctx._fid_cluster_ws = torch.empty(need, dtype=torch.uint8, device=dev)
    elif workspace.numel() * workspace.element_size() < need:
        raise ValueError('fid_cluster: the workspace holds %d bytes, %d rows need %d'
                         % (workspace.numel() * workspace.element_size(), n, need))
    ctx.check(lib().fv_fid_cluster(ctx.handle, ptr(x), n, float(eps), int(min_pts), ptr(workspace), ptr(out['labels']),
                                   ptr(out['via']), ptr(out['n_nbr']), ptr(out['core']), ptr(out['n_clusters'])), 'fv_fid_cluster')
    return out


def cluster_conf(hps):
    """hps['cluster'] -> None (absent, None or false: off) or dict(eps, min_pts, register): true takes the defaults, an object may
    carry eps (a finite number >= 0, default hps['sim_th']: a face within sim_th of a registered ID is that subject, so two faces
    within it are one person), min_pts (an int >= 1, default 3) and register (a bool, default false).  ValueError for an unknown
    key, a bool where a number is expected or a value out of range.  Needs no device."""
    c = hps.get('cluster')
    if c is None or c is False:
        return None
    if c is True:
        c = {}
    if not isinstance(c, dict):
        raise ValueError('fi_conf.hps.cluster must be true, false or an object with the keys %s, got %r' % (', '.join(CLUSTER_KEYS), c))
    unknown = sorted(set(c) - set(CLUSTER_KEYS))
    if unknown:
        raise ValueError('fi_conf.hps.cluster: unknown key %s (available: %s)' % (', '.join(map(repr, unknown)), ', '.join(CLUSTER_KEYS)))
    eps = c.get('eps', hps.get('sim_th'))
    if isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)) or not np.isfinite(eps) or eps < 0:
        raise ValueError('fi_conf.hps.cluster.eps (default: hps.sim_th) must be a finite number >= 0, got %r' % (eps,))
    min_pts = c.get('min_pts', CLUSTER_MIN_PTS)
    if isinstance(min_pts, bool) or not isinstance(min_pts, (int, np.integer)) or min_pts < 1:
        raise ValueError('fi_conf.hps.cluster.min_pts must be an int >= 1, got %r' % (min_pts,))
    register = c.get('register', False)
    if not isinstance(register, bool):
        raise ValueError('fi_conf.hps.cluster.register must be true or false, got %r' % (register,))
    return dict(eps=float(eps), min_pts=int(min_pts), register=register)


def cluster_files(resource_type):
    """The csv cluster_unknown writes for a resource type."""
    if resource_type == RESOURCE_TYPE_UCCS:
        return 'subject_clusters.csv'
    if resource_type == RESOURCE_TYPE_VGGFACE2:
        return 'subject_clusters_vggface2.csv'
    raise ValueError('resource type is not valid.')


def cluster_csv_text(names, labels, core, n_nbr, via):
    """subject_clusters.csv: one row per unlabelled face in db order; via_face_file is the face itself for a core row, the
    claiming core face for a border row and empty for noise."""
    rows = ['face_file,cluster,core,n_neighbours,via_face_file\n']
    for k, name in enumerate(names):
        rows.append('%s,%d,%d,%d,%s\n' % (name, int(labels[k]), int(core[k]), int(n_nbr[k]), names[int(via[k])] if via[k] >= 0 else ''))
    return ''.join(rows)


PAIR_TRIANGLE, PAIR_RECTANGLE = 0, 1     # fv_pair_block.kind


def pair_block_pairs(blocks):
    """Pairs of each row of a block table (k, 6) int64 (a0, na, b0, nb, out_off, kind): na(na-1)/2 or na*nb."""
    b = np.asarray(blocks, np.int64).reshape(-1, 6)
    return np.where(b[:, 5] == PAIR_TRIANGLE, b[:, 1] * (b[:, 1] - 1) // 2, b[:, 1] * b[:, 3])


def expand_pair_blocks(blocks):
    """Host expansion of a block table: -> (a rows, b rows) int64, one entry per pair in dists order (a block's pairs at
    out_off + rank, fv_fid_pair_dists' contract); slots no block writes are -1."""
    b = np.asarray(blocks, np.int64).reshape(-1, 6)
    pairs = pair_block_pairs(b)
    n = int((b[:, 4] + pairs).max()) if len(b) else 0
    ra, rb = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    for (a0, na, b0, nb, off, kind), m in zip(b.tolist(), pairs.tolist()):
        if kind == PAIR_TRIANGLE:
            i, j = np.triu_indices(na, 1)              # row-major i < j
        else:
            i, j = np.divmod(np.arange(m, dtype=np.int64), max(nb, 1))
        ra[off:off + m] = a0 + i
        rb[off:off + m] = b0 + j
    return ra, rb


def fid_pair_dists(ctx, ids, blocks, thresholds, n_dists=None, counts=None):
    """fv_fid_pair_dists: ids (n, 64) float32 CUDA tensor, blocks (k, 6) int64 rows (a0, na, b0, nb, out_off, kind), thresholds
    ascending float32 (1..4096) -> (dists float32 CUDA tensor of n_dists, or None, counts int64 CUDA tensor (2, n_th)), stream-
    ordered.  n_dists None: counts only (no distance buffer is allocated); otherwise the length of the distance buffer.  counts: an
    int64 CUDA tensor (2, n_th) to overwrite instead of a new one."""
    from ._lib import PairBlock
    x = ids.contiguous()
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != DENSE1_DIM:
        raise ValueError('fid_pair_dists expects float32 (n, 64) ids')
    b = np.ascontiguousarray(np.asarray(blocks, np.int64).reshape(-1, 6))
    th = np.ascontiguousarray(np.asarray(thresholds, np.float32).reshape(-1))
    table = (PairBlock * max(1, len(b)))()
    for k, (a0, na, b0, nb, off, kind) in enumerate(b.tolist()):
        table[k] = PairBlock(a0, na, b0, nb, off, kind, 0)
    if counts is None:
        counts = torch.empty((2, len(th)), dtype=torch.int64, device=x.device)
    dists = None if n_dists is None else torch.empty(max(1, int(n_dists)), dtype=torch.float32, device=x.device)
    ctx.check(lib().fv_fid_pair_dists(ctx.handle, ptr(x), int(x.shape[0]), table, len(b),
                                      th.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(th),
                                      None if dists is None else ptr(dists), 0 if n_dists is None else int(n_dists), ptr(counts)),
              'fv_fid_pair_dists')
    return (None if dists is None else dists[:int(n_dists)]), counts


# ----------------------------------------------------------------------------- triplet mining
MINING_MODES = {'semi_hard': 0, 'hardest': 1}                 # fv_fid_mine_negatives' mode
MINE_PB = 8                      # FV_MINE_PB of include/fv_hotpath.h: positives of one anchor that share a scan of the rows
# fv_fid_mine_negatives' kind: a negative inside the margin band, one at or nearer than the positive, one beyond the band, none
KIND_SEMI_HARD, KIND_VIOLATING, KIND_EASY, KIND_NONE = 0, 1, 2, 3


def mining_mode(hps):
    """hps['triplet_mining'] -> None (absent, None or 'none': the reference's triplets) or 'semi_hard' / 'hardest'; ValueError for
    anything else, and for a hps['mining_every'] that is not an int >= 1.  Needs no device."""
    mode = hps.get('triplet_mining')
    if mode is None or mode == 'none':
        return None
    if mode not in MINING_MODES:
        raise ValueError('fi_conf.hps.triplet_mining %r is not valid (available: none, %s)' % (mode, ', '.join(sorted(MINING_MODES))))
    every = hps.get('mining_every', 1)
    if isinstance(every, bool) or not isinstance(every, int) or every < 1:
        raise ValueError('fi_conf.hps.mining_every must be an int >= 1, got %r' % (every,))
    return mode


def refuse_mining_on_ranks(hps, ranks):
    """Mining on more than one rank is not served: every rank would have to train on the same mined list (ranks that cut it
    differently skip different batches and hang in a collective), which needs a broadcast and a run on two GPUs to prove."""
    if int(ranks) > 1 and mining_mode(hps) is not None:
        raise NotImplementedError('fi_conf.hps.triplet_mining with multi_gpu and %d ranks is not implemented: train on one GPU, '
                                  'or without mining' % int(ranks))
    # in-batch mining across ranks needs an all-gather of the facial IDs (every anchor sees the merged batch) and two GPUs to prove
    if int(ranks) > 1 and batch_mining_mode(hps) is not None:
        raise NotImplementedError('fi_conf.hps.batch_mining with multi_gpu and %d ranks is not implemented: train on one GPU, '
                                  'or without in-batch mining' % int(ranks))
    # the margin softmax across ranks needs the class gradients and the softmax sums all-reduced, and two GPUs to prove
    if int(ranks) > 1 and margin_softmax_kind(hps) is not None:
        raise NotImplementedError('fi_conf.hps.margin_softmax with multi_gpu and %d ranks is not implemented: train on one GPU, '
                                  'or without the margin softmax' % int(ranks))


def batch_mining_mode(hps):
    """hps['batch_mining'] -> None (absent, None or 'none') or 'batch_hard' / 'batch_semi_hard'; ValueError for anything else."""
    mode = hps.get('batch_mining')
    if mode is None or mode == 'none':
        return None
    if not isinstance(mode, str) or mode not in BATCH_MINING_MODES:
        raise ValueError('fi_conf.hps.batch_mining %r is not valid (available: none, %s)' % (mode, ', '.join(sorted(BATCH_MINING_MODES))))
    return mode


def _hps_int(hps, key, default, least):
    v = hps.get(key, default)
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least:
        raise ValueError('fi_conf.hps.%s must be an int >= %d, got %r' % (key, least, v))
    return int(v)


def batch_mining_conf(hps, image_size):
    """hps -> None (no in-batch mining) or dict(mode, P, K, seed): hps['batch_mining'], pk_crops (K, default 4), pk_subjects (P,
    default max(2, 3 * batch_size // K): the tower images of the reference's step), pk_seed (default 0).  ValueError for a value
    that is not served, for batch_mining together with triplet_mining, and for P * K beyond what one call takes at image_size.
    Needs no device."""
    mode = batch_mining_mode(hps)
    if mode is None:
        return None
    if mining_mode(hps) is not None:
        raise ValueError('fi_conf.hps.batch_mining and fi_conf.hps.triplet_mining are two ways to choose the negatives: set one of them')
    K = _hps_int(hps, 'pk_crops', 4, 2)
    P = _hps_int(hps, 'pk_subjects', max(2, 3 * int(hps['batch_size']) // K), 2)
    seed = _hps_int(hps, 'pk_seed', 0, 0)
    most = min(BATCH_MAX_ROWS, Model.max_infer_batch(image_size))
    if P * K > most:
        raise ValueError('fi_conf.hps: pk_subjects * pk_crops = %d images, one step at image_size %d takes at most %d'
                         % (P * K, int(image_size), most))
    return dict(mode=mode, P=P, K=K, seed=seed)


def margin_softmax_kind(hps):
    """hps['margin_softmax'] -> None (absent, None or 'none') or 'cosface' / 'arcface'; ValueError for anything else."""
    kind = hps.get('margin_softmax')
    if kind is None or kind == 'none':
        return None
    if not isinstance(kind, str) or kind not in MARGIN_SOFTMAX_KINDS:
        raise ValueError('fi_conf.hps.margin_softmax %r is not valid (available: none, %s)' % (kind, ', '.join(sorted(MARGIN_SOFTMAX_KINDS))))
    return kind


def _hps_float(hps, key, default, below):
    """A finite number in (0, below); bool and strings are refused."""
    v = hps.get(key, default)
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or not 0 < v < below:
        raise ValueError('fi_conf.hps.%s must be a number in (0, %g), got %r' % (key, below, v))
    return float(v)


def margin_softmax_conf(hps, image_size):
    """hps -> None (no margin softmax) or dict(kind, scale, margin, seed, P, K, pk_seed): hps['margin_softmax'], ms_scale (> 0,
    default 30), ms_margin (cosface: in (0, 1), default 0.35; arcface: in (0, pi / 2), default 0.5), ms_seed (the class kernel's,
    default 0) and the PK sampler's pk_crops / pk_subjects / pk_seed with batch_mining_conf's defaults and limits.  ValueError for
    a value that is not served and for margin_softmax together with batch_mining or triplet_mining.  Needs no device."""
    kind = margin_softmax_kind(hps)
    if kind is None:
        return None
    if mining_mode(hps) is not None or batch_mining_mode(hps) is not None:
        raise ValueError('fi_conf.hps.margin_softmax trains without triplets: set it without batch_mining and triplet_mining')
    scale = _hps_float(hps, 'ms_scale', MARGIN_SOFTMAX_SCALE, float('inf'))
    margin = _hps_float(hps, 'ms_margin', MARGIN_SOFTMAX_MARGINS[kind], 1.0 if kind == 'cosface' else float(np.pi / 2))
    seed = _hps_int(hps, 'ms_seed', 0, 0)
    pk = batch_mining_conf(dict(hps, batch_mining='batch_hard', triplet_mining=None), image_size)
    return dict(kind=kind, scale=scale, margin=margin, seed=seed, P=pk['P'], K=pk['K'], pk_seed=pk['seed'])


def check_class_count(C):
    if int(C) > CLASSES_MAX:
        raise ValueError('fi_conf.hps.margin_softmax: the db holds %d subjects, the class kernel takes at most %d' % (int(C), CLASSES_MAX))


def subject_list(subject_ids, codes):
    """The subject id of every class: ids[c] is the id subject_codes gave code c (int64 for UCCS, bytes for VGGFace2)."""
    C = int(codes.max()) + 1 if len(codes) else 0
    ids = [None] * C
    for sid, c in zip(subject_ids, codes.tolist()):
        if c >= 0:
            ids[c] = sid
    if all(isinstance(v, str) for v in ids):
        return np.char.encode(np.asarray(ids, dtype=str), 'utf8') if ids else np.zeros(0, 'S1')
    return np.asarray(ids, np.int64)


def pk_batches(codes, P, K, rng):
    """One epoch of PK batches (FaceNet section 3.2; Hermans et al.): codes: one subject code per db row (subject_codes), rng: a
    numpy Generator.  The subjects of a code >= 0 with at least 2 rows are shuffled and cut into groups of P (a last group of fewer
    than 2 subjects is dropped: it has no negatives); of every subject of a group min(K, its rows) rows are drawn without
    replacement -> lists of db row positions, a subject's rows side by side.  A pure function of its arguments and rng's state."""
    rows_of = {}
    for pos, c in enumerate(np.asarray(codes).tolist()):
        if c >= 0:
            rows_of.setdefault(c, []).append(pos)
    eligible = [c for c in sorted(rows_of) if len(rows_of[c]) >= 2]
    order = rng.permutation(len(eligible))
    out = []
    for g in range(0, len(order), int(P)):
        group = [eligible[j] for j in order[g:g + int(P)]]
        if len(group) < 2:
            continue
        batch = []
        for c in group:
            rows = rows_of[c]
            batch += [rows[j] for j in rng.permutation(len(rows))[:int(K)]]
        out.append(batch)
    return out


def subject_codes(subject_ids):
    """Subject ids of a db (ints for UCCS, strings for VGGFace2) -> int32 codes for fv_fid_mine_negatives: -1 stays -1 (an unknown
    identity), every other id gets the position of its first appearance."""
    code, out = {}, np.empty(len(subject_ids), np.int32)
    for k, sid in enumerate(subject_ids):
        if not isinstance(sid, str) and sid == -1:
            out[k] = -1
        else:
            out[k] = code.setdefault(sid, len(code))
    return out


def triplet_groups(pairs, sort=False):
    """(anchor slot, positive slot) pairs -> (anchors, pos_off, positives, order), fv_fid_mine_negatives' group table: every run
    of consecutive equal anchors is one group (an anchor that recurs later starts another).  Output j of the operator belongs to
    pairs[order[j]].  sort: the pairs are first ordered by anchor (stably), so that every anchor is one group whatever the order
    of the list -- the operator's outputs do not depend on the grouping, only its time does."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    order = np.argsort(pairs[:, 0], kind='stable') if sort else np.arange(len(pairs))
    a, p = pairs[order, 0], pairs[order, 1]
    starts = np.flatnonzero(np.concatenate([[True], a[1:] != a[:-1]])) if len(a) else np.zeros(0, np.int64)
    pos_off = np.concatenate([starts, [len(a)]]).astype(np.int32)
    return a[starts].astype(np.int32), pos_off, p.astype(np.int32), order.astype(np.int64)


def mined_rows(pairs_labels, neg_slot, kind, labels, drop_easy):
    """The triplet rows -- (anchor, positive, negative) labels -- train() cuts into batches: pair k of pairs_labels with the
    label of slot neg_slot[k]; a pair without a negative (KIND_NONE) is left out, with drop_easy also one whose negative lies
    beyond the margin (KIND_EASY: loss 0, gradient 0)."""
    out = []
    for (a, p), n, k in zip(pairs_labels, neg_slot, kind):
        if k == KIND_NONE or (drop_easy and k == KIND_EASY):
            continue
        out.append((a, p, labels[int(n)]))
    return out


def fid_mine_negatives(ctx, ids, subjects, anchors, pos_off, positives, margin=TRIPLET_MARGIN, mode='semi_hard'):
    """fv_fid_mine_negatives: ids (n, 64) float32 and subjects (n,) int32 CUDA tensors, the group table anchors (g,), pos_off
    (g + 1,), positives (t,) int32 on the host -> (neg_index int32, kind int32, d_ap float64, d_an float64) CUDA tensors of t
    (stream-ordered).  mode: 'semi_hard' / 'hardest' (or 0 / 1)."""
    if not torch.is_tensor(ids) or ids.dtype != torch.float32 or ids.dim() != 2 or ids.shape[1] != DENSE1_DIM:
        raise ValueError('fid_mine_negatives expects float32 (n, 64) ids')
    if not torch.is_tensor(subjects) or subjects.dtype != torch.int32 or subjects.shape != (ids.shape[0],):
        raise ValueError('fid_mine_negatives expects int32 (n,) subjects, one per row of ids')
    table = []
    for name, v in (('anchors', anchors), ('pos_off', pos_off), ('positives', positives)):
        v = np.asarray(v)
        if v.dtype != np.int32 or v.ndim != 1:
            raise ValueError('fid_mine_negatives expects a one-dimensional int32 array as %s' % name)
        table.append(np.ascontiguousarray(v))
    a, off, pos = table
    if len(off) != len(a) + 1:
        raise ValueError('fid_mine_negatives expects one offset per group and one more (%d groups, %d offsets)' % (len(a), len(off)))
    mode = MINING_MODES.get(mode, mode) if isinstance(mode, str) else mode
    if isinstance(mode, bool) or not isinstance(mode, int):
        raise ValueError('fid_mine_negatives: mode %r (available: %s)' % (mode, ', '.join(sorted(MINING_MODES))))
    if not ids.is_cuda or subjects.device != ids.device or ids.device.index != ctx.device:
        raise ValueError('fid_mine_negatives expects ids and subjects on the context\'s device (cuda:%d)' % ctx.device)
    x, sub = ids.contiguous(), subjects.contiguous()
    t = len(pos)
    neg = torch.empty(t, dtype=torch.int32, device=x.device)
    kind = torch.empty(t, dtype=torch.int32, device=x.device)
    d_ap = torch.empty(t, dtype=torch.float64, device=x.device)
    d_an = torch.empty(t, dtype=torch.float64, device=x.device)
    i32p = ctypes.POINTER(ctypes.c_int32)
    ctx.check(lib().fv_fid_mine_negatives(ctx.handle, ptr(x), ptr(sub), int(x.shape[0]), a.ctypes.data_as(i32p),
                                          off.ctypes.data_as(i32p), len(a), pos.ctypes.data_as(i32p), t, float(margin), mode,
                                          ptr(neg), ptr(kind), ptr(d_ap), ptr(d_an)), 'fv_fid_mine_negatives')
    return neg, kind, d_ap, d_an


from .postproc import letterbox_crops      # noqa: E402, F401 (lives next to the other letterbox wrappers; FaceDetector's tiles use it too)


def crop_nearest_u8(ctx, images, crops, image_size, out=None):
    """fv_crop_nearest_u8: images and crops as for letterbox_crops -> (n, S, S, 3) uint8 CUDA tensor, each crop resized by
    nearest neighbour to its letterbox size and zero padded (create_db_fi's cv.resize(INTER_NEAREST) + cv.copyMakeBorder)."""
    n, S = len(crops), int(image_size)
    if out is None:
        out = torch.empty((n, S, S, 3), dtype=torch.uint8, device=images[0].device)
    flat = [int(v) for c in crops for v in c]
    rc = lib().fv_crop_nearest_u8(ctx.handle, *packed_args(*images), (ctypes.c_int32 * max(1, 5 * n))(*flat), n, S, ptr(out))
    ctx.check(rc, 'fv_crop_nearest_u8')
    return out


GATHER_CHUNK = 128               # FV_GATHER_CHUNK of include/fv_hotpath.h: indices per launch of fv_gather_u8_f32


def gather_crops_f32(ctx, store, idx, out=None):
    """fv_gather_u8_f32: store (N, ...) uint8 CUDA tensor, idx int sequence -> (n, ...) float32 CUDA tensor, out[j] = store[idx[j]]
    / 255 (correctly rounded; stream-ordered).  A slot's byte count must be a multiple of 16."""
    idx = np.ascontiguousarray(np.asarray(idx).reshape(-1), np.int32)
    if store.dtype != torch.uint8 or not store.is_cuda or store.dim() < 2:
        raise ValueError('gather_crops_f32 expects a uint8 CUDA tensor of slots')
    n, elems = len(idx), int(np.prod(store.shape[1:]))
    if out is None:
        out = torch.empty((n,) + tuple(store.shape[1:]), dtype=torch.float32, device=store.device)
    elif out.dtype != torch.float32 or out.device != store.device or out.numel() != n * elems:
        raise ValueError('gather_crops_f32: out must be a float32 tensor of %d x %d elements on the store\'s device' % (n, elems))
    rc = lib().fv_gather_u8_f32(ctx.handle, ptr(store), int(store.shape[0]), elems, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                n, ptr(out))
    ctx.check(rc, 'fv_gather_u8_f32')
    return out


def draw_prims_u8(ctx, images, prims, masks):
    """fv_draw_prims_u8: draw the annotate.Outline / annotate.MaskBlend records `prims`, in order, onto images = (device uint8
    buffer, offsets, hw) of a batch, in place (stream-ordered).  masks: uint8 CUDA tensor the MaskBlend offsets point into
    (annotate.pack_masks), or None when there is no MaskBlend.  A bad record raises FvError and nothing is drawn."""
    from ._lib import DrawPrim
    dbuf, offs, hw = images
    n, ni = len(prims), len(offs)
    if n == 0:
        return
    if dbuf.dtype != torch.uint8 or not dbuf.is_cuda or (masks is not None and (masks.dtype != torch.uint8 or not masks.is_cuda)):
        raise ValueError('draw_prims_u8 expects uint8 CUDA tensors')
    for i in range(ni):
        if offs[i] < 0 or offs[i] + max(0, hw[2 * i]) * max(0, hw[2 * i + 1]) * 3 > dbuf.numel():
            raise ValueError('draw_prims_u8: image %d lies outside the buffer' % i)
    table = (DrawPrim * n)()
    for k, p in enumerate(prims):
        if isinstance(p, Outline):
            v = (0, p.image, p.x0, p.y0, p.x1, p.y1, p.width) + tuple(p.color) + (0, 0)
        else:
            v = (1, p.image, p.x, p.y, p.mw, p.mh, 0) + tuple(p.color) + (0, p.mask_off)
        v = tuple(int(a) for a in v)
        if not all(-2 ** 31 <= a < 2 ** 31 for a in v[:7]) or not all(0 <= c <= 255 for c in v[7:10]):
            raise ValueError('draw_prims_u8: primitive %d out of range: %r' % (k, p))
        table[k] = DrawPrim(*v)
    rc = lib().fv_draw_prims_u8(ctx.handle, *packed_args(dbuf, offs, hw), table, n,
                                None if masks is None else ptr(masks), 0 if masks is None else masks.numel())
    ctx.check(rc, 'fv_draw_prims_u8')


def ground_truth_boxes(df):
    """The ground-truth boxes evaluate() draws for one frame's rows of validation.csv (fi.py:956-969), filtered as
    FaceDetector.evaluate filters them: a row counts only when FACE_X, FACE_Y, FACE_WIDTH and FACE_HEIGHT are all > 0; the box is
    int(x), int(y), int(x + w - 1), int(y + h - 1) and carries the row's SUBJECT_ID."""
    from .postproc import BoundBox
    out = []
    for i in range(df.shape[0]):
        x, y, w, h = df.iloc[i, 3:7].values.astype(np.float64)
        if not (x > 0 and y > 0 and w > 0 and h > 0):
            continue
        out.append(BoundBox(int(x), int(y), int(x + w - 1), int(y + h - 1), objness=1., classes=[1.0], subject_id=df.iloc[i, 2]))
    return out


def save_frame(pixels, path):
    from PIL import Image
    Image.fromarray(pixels).save(path)


# ----------------------------------------------------------------------------- data mode (fi.py:78-280)
# One face crop to cut: the source image, the rectangle (y0, x0, rows, cols) inside it, the file name under the faces directory
# and the db row (subject_id, face_file, w, h) -- w, h of the cut crop, not of the csv's box.
CropRecord = collections.namedtuple('CropRecord', 'source rect name row')

DATA_BATCH_BYTES = 192 << 20     # decoded RGB per batch: three 18-megapixel UCCS frames (their coefficients take as much again)
DATA_BATCH_CROPS = 256           # crops per batch: 133 MB of output at 416, on the device and in each pinned slot


def image_hw(path):
    """(rows, columns) from the file's header; the pixels are not decoded."""
    from PIL import Image
    with Image.open(path) as im:
        return im.size[1], im.size[0]


def _keep(records, skipped, source, rect, name, subject_id, image_size):
    if rect is None:
        skipped['empty'] += 1
    elif not lb_side_ok(rect[2], rect[3], image_size):
        skipped['side_rounds_to_0'] += 1
    else:
        records.append(CropRecord(source, rect, name, (subject_id, name, rect[3], rect[2])))


def uccs_records(raw_data_path, image_size, hw_of=image_hw):
    """The crops create_db_fi cuts for UCCS (fi.py:92-167), in its order: training/training.csv grouped by SUBJECT_ID, the
    subjects walked sorted, -1 skipped, a row skipped unless FACE_X, FACE_Y, FACE_WIDTH and FACE_HEIGHT are all > 0, the cut
    `image[(t - 1):(b - 1), (l - 1):(r - 1)]` with l, t = int(x), int(y) and r, b = int(x + w - 1), int(y + h - 1).
    -> (records, skipped): skipped counts the rows whose cut is empty or whose letterboxed side rounds to 0 (the reference
    raises on those).  Reads the csv and, through hw_of(path), the image sizes; nothing else."""
    import pandas as pd
    gt = pd.read_csv(os.path.join(raw_data_path, 'training', 'training.csv'))
    records, skipped, sizes = [], {'empty': 0, 'side_rounds_to_0': 0}, {}
    for k, df in gt.groupby('SUBJECT_ID'):
        if k == -1:
            continue
        for file_name, x, y, w, h in zip(df.iloc[:, 1], df.iloc[:, 3], df.iloc[:, 4], df.iloc[:, 5], df.iloc[:, 6]):
            if not (x > 0 and y > 0 and w > 0 and h > 0):
                continue
            source = os.path.join(raw_data_path, 'training', file_name)
            if source not in sizes:
                sizes[source] = hw_of(source)
            l, t, r, b = int(x), int(y), int(x + w - 1), int(y + h - 1)
            stem, ext = os.path.splitext(file_name)
            name = stem + '_' + str(k) + '_' + str(int(x)) + '_' + str(int(y)) + ext
            _keep(records, skipped, source, slice_rect(t - 1, b - 1, l - 1, r - 1, *sizes[source]), name, k, image_size)
    return records, skipped


def vggface2_records(raw_data_path, image_size, hw_of=image_hw):
    """The crops save_extracted_face cuts for VGGFace2 (fi.py:212-280), in loose_bb_train.csv's row order: a row with x < 0,
    y < 0, w <= 0 or h <= 0 skipped, the cut `image[y:(y + h), x:(x + w)]` of train/<identity>/<file>.jpg clipped by the image,
    saved as <identity>_<file>.jpg.  -> (records, skipped) as uccs_records."""
    import pandas as pd
    df = pd.read_csv(os.path.join(raw_data_path, 'loose_bb_train.csv'))
    records, skipped, sizes = [], {'empty': 0, 'side_rounds_to_0': 0}, {}
    for name_id, x, y, w, h in zip(df.iloc[:, 0], df.iloc[:, 1], df.iloc[:, 2], df.iloc[:, 3], df.iloc[:, 4]):
        if x < 0 or y < 0 or w <= 0 or h <= 0:
            continue
        identity, file_name = name_id.split('/')[0], name_id.split('/')[1] + '.jpg'
        source = os.path.join(raw_data_path, 'train', identity, file_name)
        if source not in sizes:
            sizes[source] = hw_of(source)
        x, y, w, h = int(x), int(y), int(w), int(h)
        _keep(records, skipped, source, slice_rect(y, y + h, x, x + w, *sizes[source]), identity + '_' + file_name, identity,
              image_size)
    return records, skipped


def db_csv_text(records):
    """The subject db as the reference's `db.to_csv()` writes it: the index column first -- every row's label is 0, each row
    having been a one-row frame of its own before pd.concat -- then subject_id, face_file, w, h."""
    f = io.StringIO()
    out = csv.writer(f, lineterminator='\n')
    out.writerow(['', 'subject_id', 'face_file', 'w', 'h'])
    for r in records:
        out.writerow([0] + list(r.row))
    return f.getvalue()


def source_batches(records, hw_of, batch_bytes=DATA_BATCH_BYTES, batch_crops=DATA_BATCH_CROPS):
    """Group the records by source file (files in order of first appearance) and the files into batches of at most
    batch_bytes of decoded RGB and batch_crops crops -- a single file beyond either makes a batch of its own.
    -> [[(source, [record index, ...]), ...], ...]"""
    by_source = collections.OrderedDict()
    for i, r in enumerate(records):
        by_source.setdefault(r.source, []).append(i)
    batches, cur, nbytes, ncrops = [], [], 0, 0
    for source, idx in by_source.items():
        h, w = hw_of(source)
        if cur and (nbytes + h * w * 3 > batch_bytes or ncrops + len(idx) > batch_crops):
            batches.append(cur); cur, nbytes, ncrops = [], 0, 0
        cur.append((source, idx)); nbytes += h * w * 3; ncrops += len(idx)
    if cur:
        batches.append(cur)
    return batches


def load_batch(files, pool, ring, device_jpeg=True):
    """Host half of a batch's decode, as FaceDetector._detect_files does it: the files Huffman-decoded on `pool` into a pinned
    slot of `ring` -> ('jpeg', int16 coefficients, jpeg.BatchPlan); when the parser refuses one of them (progressive, CMYK, ...)
    or the scan data are damaged, the batch decoded by Pillow -> pack_images' (buffer, offsets, hw)."""
    from . import jpeg
    from .face_detection import map_all
    from .postproc import pack_images
    if device_jpeg:
        datas = list(pool.map(lambda f: open(f, 'rb').read(), files))
        infos = [jpeg.parse(d) for d in datas]
        if all(i is not None for i in infos):
            plan = jpeg.BatchPlan(infos)
            buf = ring.take(2 * plan.total_coefs).view(torch.int16)
            view = buf.numpy()
            try:
                map_all(pool, lambda i: jpeg.entropy_decode(datas[i], infos[i],
                                                            view[plan.coef_off[i]:plan.coef_off[i] + int(infos[i].total_coefs)]),
                        range(len(files)))
                return 'jpeg', buf, plan
            except ValueError:
                ring.untake()
    return pack_images(list(pool.map(_imread, files)), ring=ring)


def stage_batch(ctx, loaded, ring, device):
    """Device half: the host-to-device copy and, for a 'jpeg' batch, fv_jpeg_reconstruct_batch -> (device uint8 buffer, offsets,
    hw), the packed RGB images as fv_crop_nearest_u8 reads them."""
    from . import jpeg
    if isinstance(loaded[0], str):
        _tag, coefs, plan = loaded
        images = (jpeg.reconstruct_batch(ctx, plan, coefs.to(device, non_blocking=True), device), plan.rgb_off, plan.hw)
        ring.copied(coefs)
    else:
        buf, offs, hw = loaded
        images = (buf.to(device, non_blocking=True), offs, hw)
        ring.copied(buf)
    return images


def write_crop(pixels, path):
    from PIL import Image
    Image.fromarray(pixels).save(path)


def write_bytes(data, path):
    with open(path, 'wb') as f:
        f.write(data)


# device_encode where a configuration does not say: on -- the files are the same bytes, and DESIGN.md section 18 gives the
# measurements behind the choice
DEVICE_ENCODE_DEFAULT = True
# crop_store where a configuration does not say: on -- train() and the facial-ID database read their crops from a device-resident
# store (crop_store.py); the inputs are the same bits, and DESIGN.md section 19 gives the measurements
CROP_STORE_DEFAULT = True


def encode_on_device(device_encode, h, w):
    """Whether an h x w image of a batch is encoded by jpeg.encode_batch: only when the caller asked for it, and only sizes a
    JPEG's 16-bit fields hold (an image taller or wider than 65535 pixels goes to Pillow, whose error is then the user's)."""
    from . import jpeg
    return bool(device_encode) and jpeg.can_encode(h, w)


def cut_and_write(ctx, records, image_size, out_dir, threads, hw_of=image_hw, device_jpeg=True, batch_bytes=DATA_BATCH_BYTES,
                  batch_crops=DATA_BATCH_CROPS, device_encode=DEVICE_ENCODE_DEFAULT):
    """Cut every record's crop and write it to out_dir/<name>.  Per batch of source files: decode (load_batch on a loader thread,
    stage_batch), ONE fv_crop_nearest_u8 call for all its crops, the S x S x 3 uint8 crops copied to a pinned buffer, then
    encoded and written by Pillow on the thread pool while the next batch decodes.  device_encode: the crops are encoded where
    they lie (jpeg.encode_batch), only the files' bytes -- the same bytes -- cross into the pinned slot, and the pool just writes
    them."""
    from concurrent.futures import ThreadPoolExecutor, wait
    from .postproc import PinnedRing
    S = int(image_size)
    dev = torch.device('cuda', ctx.device)
    batches = source_batches(records, hw_of, batch_bytes, batch_crops)
    if not batches:
        return
    ring = PinnedRing(3)
    outs = [[None, []], [None, []]]              # two pinned output slots: (buffer, the writes still reading it)
    with ThreadPoolExecutor(max_workers=threads) as pool, ThreadPoolExecutor(max_workers=1) as one:
        pending = one.submit(load_batch, [s for s, _ in batches[0]], pool, ring, device_jpeg)
        writes = []
        for k, batch in enumerate(batches):
            loaded = pending.result()
            if k + 1 < len(batches):
                pending = one.submit(load_batch, [s for s, _ in batches[k + 1]], pool, ring, device_jpeg)
            images = stage_batch(ctx, loaded, ring, dev)
            idx = [i for _, ii in batch for i in ii]
            crops = [(f,) + tuple(records[i].rect) for f, (_, ii) in enumerate(batch) for i in ii]
            cut = crop_nearest_u8(ctx, images, crops, S)
            slot = outs[k % 2]
            wait(slot[1])                         # the writes of batch k - 2 have let go of the slot
            if encode_on_device(device_encode, S, S):
                from . import jpeg

                def pinned(nbytes, slot=slot):
                    if slot[0] is None or slot[0].numel() < nbytes:
                        slot[0] = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8).pin_memory()
                    return slot[0]
                files = jpeg.encode_batch(ctx, cut.view(-1), [j * S * S * 3 for j in range(len(crops))], [S, S] * len(crops), dev,
                                          pinned=pinned)
                slot[1] = [pool.submit(write_bytes, files[j], os.path.join(out_dir, records[i].name)) for j, i in enumerate(idx)]
                writes += slot[1]
                continue
            if slot[0] is None or slot[0].shape[0] < len(crops):
                slot[0] = torch.empty((max(len(crops), min(batch_crops, len(records))), S, S, 3), dtype=torch.uint8).pin_memory()
            host = slot[0][:len(crops)]
            host.copy_(cut, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
            pixels = host.numpy()
            slot[1] = [pool.submit(write_crop, pixels[j], os.path.join(out_dir, records[i].name)) for j, i in enumerate(idx)]
            writes += slot[1]
        wait(writes)
        for w in writes:
            w.result()


def create_db_fi(conf, device=None):
    """The data mode (fi.py:78-210): cut every face of the resource's ground truth, letterbox it to image_size by nearest
    neighbour and write it under <raw_data_path>/subject_faces/ (vggface2: subject_faces_vggface2/), emptied first; write the
    subject db (subject_image_db.csv / subject_image_vggface2_db.csv) in the reference's row order.  A source image is decoded
    once for all its faces (cut_and_write).  Rows the reference would raise on are skipped and counted.
    -> {'written': crops, 'empty': ..., 'side_rounds_to_0': ...}"""
    conf = conf['fi_conf']
    db_file, faces_dir = db_files(conf['resource_type'])[:2]
    raw_data_path = conf['raw_data_path']
    S = int(conf['nn_arch']['image_size'])
    if S % 32 or S < 32:
        raise ValueError('image_size must be a positive multiple of 32 (network stride)')
    if device is None:
        device = int(os.environ.get('FV_DEVICE', os.environ.get('LOCAL_RANK', 0)))
    ctx = Context(device)                  # no GPU, no data mode -- found out before the faces directory is emptied
    out_dir = os.path.join(raw_data_path, faces_dir)
    if os.path.isdir(out_dir):
        shutil.rmtree(out_dir)
    os.mkdir(out_dir)
    sizes = {}

    def hw_of(path):
        if path not in sizes:
            sizes[path] = image_hw(path)
        return sizes[path]
    enumerate_records = uccs_records if conf['resource_type'] == RESOURCE_TYPE_UCCS else vggface2_records
    records, skipped = enumerate_records(raw_data_path, S, hw_of)
    from .face_detection import default_loader_threads
    hps = conf.get('hps', {})
    cut_and_write(ctx, records, S, out_dir, max(1, int(hps.get('loader_threads', default_loader_threads()))), hw_of,
                  bool(hps.get('device_jpeg', True)), device_encode=bool(hps.get('device_encode', DEVICE_ENCODE_DEFAULT)))
    with open(db_file, 'w') as f:
        f.write(db_csv_text(records))
    print('Saved %d face images to %s; skipped %d empty crops and %d whose letterboxed side rounds to 0.'
          % (len(records), out_dir, skipped['empty'], skipped['side_rounds_to_0']))
    return dict(skipped, written=len(records))


# ----------------------------------------------------------------------------- FaceIdentifier (fi.py:288-643)
class FaceIdentifier(object):
    """Face identifier on the Darknet-53 base of YOLOv3."""

    MODEL_PATH = 'face_identifier.h5'
    CLASSES_PATH = 'face_identifier_classes.h5'    # the margin softmax's class kernel and the subject id of every class
    BASE_MODEL_PATH = 'yolov3_base.h5'
    DARKNET_WEIGHTS_PATH = 'yolov3.weights'

    TrainingSequence = TrainingSequence
    TrainingSequenceVGGFace2 = TrainingSequenceVGGFace2

    def __init__(self, conf, device=None):
        self._full_conf = conf
        self.conf = conf['fi_conf']
        self.raw_data_path = self.conf['raw_data_path']
        self.hps = self.conf['hps']
        self.nn_arch = self.conf['nn_arch']
        self.model_loading = self.conf['model_loading']
        self.image_size = int(self.nn_arch['image_size'])
        if self.image_size % 32 or self.image_size < 32:
            raise ValueError('image_size must be a positive multiple of 32 (network stride)')
        if int(self.nn_arch['dense1_dim']) != DENSE1_DIM:
            raise ValueError('dense1_dim must be %d: the triplet loss slices 0:64 / 64:128 / 128:192 (reference triplet_loss)'
                             % DENSE1_DIM)
        # multi_gpu: one process per GPU (main() starts them); a FaceIdentifier made in a process without WORLD_SIZE is one rank
        self.world = int(os.environ.get('WORLD_SIZE', 1)) if self.conf.get('multi_gpu') else 1
        self.rank = int(os.environ.get('RANK', 0)) if self.world > 1 else 0
        self.mining = mining_mode(self.hps)          # ValueError for a value that is not served, before a device is touched
        self.last_mining = None
        self.batch_mining = batch_mining_conf(self.hps, self.image_size)       # likewise
        self.last_batch_mining = None
        self.margin_softmax = margin_softmax_conf(self.hps, self.image_size)   # likewise
        self.last_margin_softmax = None
        self.cluster = cluster_conf(self.hps)                                  # likewise
        if self.margin_softmax is not None:
            self._check_db_classes()
        if device is None:           # FV_DEVICE: several ranks on ONE device, to rehearse N > 1 on a one-GPU box (gloo transport)
            device = int(os.environ.get('FV_DEVICE', os.environ.get('LOCAL_RANK', 0)))
        self.model = FidModel(self.image_size, device)
        self.model.bn_zero_debias = bool(self.conf.get('bn_zero_debias', True))
        if self.model_loading:
            self.model.load(self.MODEL_PATH)
        else:
            self._load_base()
            self.model.init_dense()
        self._fd = None
        self.fid_extractor = FidExtractor(self.model)

    @property
    def fd(self):
        """The FaceDetector of fd_conf (fi.py:374), created on first use."""
        if self._fd is None:
            from .face_detection import FaceDetector
            self._fd = FaceDetector(self._full_conf['fd_conf'])
        return self._fd

    def _check_db_classes(self):
        """ValueError when the subject db (read when it is there; train() checks the sequence's in any case) holds more subjects
        than the class kernel takes."""
        import pandas as pd
        db_file = db_files(self.conf.get('resource_type'))
        if db_file is not None and os.path.exists(db_file[0]):
            sids = pd.read_csv(db_file[0]).iloc[:, 1:]['subject_id']
            check_class_count(int(sids[sids != -1].nunique()))

    def _load_base(self):
        """YOLOV3Base (fi.py:398-614), as FaceDetector._load_base: yolov3_base.h5 when yolov3_base_model_load is set, else the
        Darknet file (then yolov3_base.h5 is written, fi.py:612), else synthetic weights (announced)."""
        base = weights.load_base('FaceIdentifier', self.model.layers, self.BASE_MODEL_PATH, self.DARKNET_WEIGHTS_PATH,
                                 self.conf.get('yolov3_base_model_load'), save_base=self.rank == 0)
        if base is None:
            self.model.init_synthetic(seed=7)
        else:
            self.model.set_base(*base)

    def create_face_reconst_model(self, seed=None):
        """fi.py:1155-1488: with fi_conf['face_vijana_recon_load'] (a missing key means false) self.recon_model is read from
        face_vijnana_recon.h5; otherwise it is built from the current model (ReconModel.from_identifier: a copy, with the dense
        bias drawn from np.random.RandomState(seed)) and that file is written.  The reference reads the file with Keras'
        load_model; a Keras-written full-model file is not served here: the file read is the weight
        layout ReconModel.save writes.  Raises ValueError without a model."""
        if not isinstance(getattr(self, 'model', None), FidModel):
            raise ValueError('A valid model instance doesn\'t exist.')
        if self.conf.get('face_vijana_recon_load'):
            self.recon_model = ReconModel(self.image_size, ctx=self.model.ctx)
            self.recon_model.load(RECON_MODEL_PATH)
            return
        self.recon_model = ReconModel.from_identifier(self.model, seed)
        self.recon_model.save(RECON_MODEL_PATH)

    def train_on_batch(self, xa, xp, xn):
        """One Keras train_on_batch of the triplet model: fv_fid_train_step, then Adam with fi_conf.hps.  Returns the loss (float)."""
        h = self.hps
        loss = self.model.train_on_batch(xa, xp, xn, h['lr'], h['beta_1'], h['beta_2'], h.get('decay', 0.0))
        return float(loss.item())

    def _loader_threads(self):
        from .face_detection import default_loader_threads
        return max(1, int(self.hps.get('loader_threads', default_loader_threads())))

    def _triplet_inputs(self, tr_gen):
        """crop_store.TripletInputs over the sequence's db (hps['crop_store'], on by default; hps['crop_store_mb'] bounds the
        resident store, 0 forces the per-batch tier), or None: the sequence's own load().  The training workspace of the first
        batch is allocated first, so that the default budget -- half of what is free -- is taken from what training leaves."""
        if not self.hps.get('crop_store', CROP_STORE_DEFAULT):
            return None
        from .crop_store import TripletInputs, store_budget
        m = self.model
        first = slice_triplets(tr_gen.rows(0), self.world, self.rank) if len(tr_gen) else None
        if first is not None and len(first[0]):
            m.ensure_optimizer()
            m._workspace(len(first[0]), self.image_size, True)
        return TripletInputs(m.ctx, m.dev, self.image_size, list(tr_gen.db.index), tr_gen.path, tr_gen.batch_size,
                             store_budget(self.hps, m.dev), self._loader_threads())

    def train(self):
        """fi.py:616-643: fit_generator over the triplet sequence (batch order shuffled every epoch, as Keras does for a Sequence),
        hps['epochs'] epochs of hps['step'] steps (the sequence sets hps['step'] to its batch count), then save face_identifier.h5.
        With more than one rank (multi_gpu): rank 0 builds, shuffles and pickles the triplet list and the others read it; every
        rank walks the same batch order and trains on its slice of each batch (slice_triplets) through
        parallel.DataParallelTrainer; a batch with fewer triplets than ranks is skipped on all ranks; rank 0 prints the loss of
        the merged batches and saves the model.
        hps['triplet_mining'] ('semi_hard' / 'hardest'; one rank only): at the start of every epoch e with e % hps['mining_every']
        == 0 (default 1) the negatives are mined anew (mine_triplets; hps['mining_drop_easy'], default true, leaves out the
        triplets whose loss is already 0) and one line is printed; the epoch's batches are cut from the mined rows as rows()
        cuts the sequence's list, and min(hps['step'], batches) of them run in shuffled order.  The pickle stays the reference's
        list.  Without the key nothing here differs from the above."""
        from .parallel import DataParallelTrainer
        refuse_mining_on_ranks(self.hps, self.world)
        sequence = self._sequence()
        trainer = DataParallelTrainer(self.model, world_size=self.world, rank=self.rank)
        # one triplet list for all ranks: rank 0 writes the pickle, the others load it once it is complete
        if self.rank == 0:
            tr_gen = sequence(self.raw_data_path, self.hps, self.nn_arch, load_flag=False)
        trainer.barrier()
        if self.rank != 0:
            tr_gen = sequence(self.raw_data_path, self.hps, self.nn_arch, load_flag=True)
        h = self.hps
        steps, epochs = int(h['step']), int(h['epochs'])
        pk = batch_mining_conf(h, self.image_size) if batch_mining_mode(h) is not None else None
        if pk is not None:                 # one rank (refused above otherwise): no collective in the loop
            self._train_pk(tr_gen, pk, steps, epochs)
        elif margin_softmax_kind(h) is not None:      # one rank as well
            self._train_classes(tr_gen, margin_softmax_conf(h, self.image_size), steps, epochs)
        else:
            self._train_triplets(tr_gen, trainer, steps, epochs)
        if self.rank == 0:
            print('Save the model.')
            self.model.save(self.MODEL_PATH)
        trainer.shutdown()

    def _train_triplets(self, tr_gen, trainer, steps, epochs):
        """train() over the sequence's triplets (mined anew where hps['triplet_mining'] says so), on every rank."""
        h = self.hps
        inputs = self._triplet_inputs(tr_gen)
        # one rank: the global numpy stream, as before; several: one seeded generator, the same batch order on every rank
        rng = np.random.default_rng(0) if self.world > 1 else np.random
        try:
            batch_rows, n_batches = tr_gen.rows, len(tr_gen)
            for e in range(epochs):
                losses = []
                if self.mining is not None and e % int(h.get('mining_every', 1)) == 0:
                    mined, _ = self.mine_triplets(bool(h.get('mining_drop_easy', True)), tr_gen, inputs)
                    bs, c = tr_gen.batch_size, self.last_mining['counts']
                    print('Mining (%s) - semi-hard: %d, violating: %d, easy: %d, no negative: %d - %.3fs'
                          % (self.mining, c[0], c[1], c[2], c[3], self.last_mining['seconds']))
                    batch_rows, n_batches = (lambda i, mined=mined, bs=bs: mined[i * bs:(i + 1) * bs]), num_batches(len(mined), bs)
                order = [int(i) for i in rng.permutation(n_batches)[:steps]]
                parts = [slice_triplets(batch_rows(i), self.world, self.rank) for i in order]
                # crop_store: this epoch's inputs come from the store, in step order (per batch: the next one decodes meanwhile)
                feed = None if inputs is None else inputs.batches([part[0] for part in parts if part is not None])
                for i, part in zip(order, parts):
                    if part is None:       # on every rank alike: a rank that stayed out of a collective would hang the others
                        if self.rank == 0:
                            print('batch %d - skipped (fewer triplets than ranks)' % i)
                        continue
                    rows, weight = part
                    if feed is None:
                        x, _ = tr_gen.load(rows)
                        xs = (x['input_a'], x['input_p'], x['input_n'])
                    else:
                        xs = next(feed)
                    loss = trainer.train_on_inputs(xs, h['lr'], h['beta_1'], h['beta_2'], h.get('decay', 0.0), weight=weight)
                    losses.append(trainer.merged_loss(loss, weight))          # collective: every rank calls it
                if self.rank == 0:
                    print('Epoch %d/%d - loss: %.4f' % (e + 1, epochs, float(np.mean(losses)) if losses else float('nan')))
        finally:
            if inputs is not None:
                inputs.close()

    def _train_pk(self, tr_gen, pk, steps, epochs):
        """train() with hps['batch_mining']: every epoch draws its PK batches (pk_batches, one generator
        seeded with pk_seed for the whole run -- never the global stream), runs min(steps, batches) of them through
        FidModel.train_on_labelled_batch, the crops fed by TripletInputs.crop_batches, and prints the mean loss and, summed over
        the epoch, the anchors of each kind and how many had a hinge that passes a gradient.  Nothing is read back before the
        epoch's last step is in the queue.  self.last_batch_mining: the batches (db row positions) of every epoch, the last
        epoch's counts."""
        m, h = self.model, self.hps
        last = self.last_batch_mining = dict(batches=[], counts=None, active=None)
        sums = torch.zeros(5, dtype=torch.int64, device=m.dev)        # this epoch's anchors of each kind, active hinges

        def step(x, subjects):
            loss = m.train_on_labelled_batch(x, subjects, pk['mode'], h['lr'], h['beta_1'], h['beta_2'], h.get('decay', 0.0))
            sel = m.batch_selection
            valid = sel['kind'] != KIND_NONE
            sums[:4] += torch.bincount(sel['kind'].to(torch.int64), minlength=4)[:4]
            sums[4] += (valid & (sel['d_ap'] - sel['d_an'] + TRIPLET_MARGIN >= 0)).sum()     # NaN >= 0 is False
            return loss

        def report(e, mean):
            c = [int(v) for v in sums.cpu()]
            sums.zero_()
            last.update(counts=c[:4], active=c[4])
            print('Epoch %d/%d - loss: %.4f - anchors (%s) semi-hard: %d, violating: %d, easy: %d, without a triplet: %d, active: %d'
                  % (e + 1, epochs, mean, pk['mode'], c[0], c[1], c[2], c[3], c[4]))
        self._train_labelled(tr_gen, pk['P'], pk['K'], pk['seed'], steps, epochs, last['batches'], m._batch_workspace, step, report)

    def _train_labelled(self, tr_gen, P, K, seed, steps, epochs, drawn, workspace, step, report):
        """The loop of _train_pk and _train_classes.  workspace(P * K) allocates the step's workspace, before the store's budget is
        taken from what is free; the crops come from a TripletInputs (hps['crop_store']: the store, else the host tier).  Every
        epoch draws its batches of db row positions (pk_batches, one generator seeded with `seed` for the whole run), appends
        them to `drawn`, runs min(steps, batches) of them through step(x, codes) -> loss and calls report(e, mean loss) once
        the epoch's last step is in the queue: nothing is read back before."""
        from .crop_store import HOST, TripletInputs, store_budget
        m, h = self.model, self.hps
        labels = list(tr_gen.db.index)
        codes = subject_codes(list(tr_gen.db['subject_id']))
        rng = np.random.default_rng(seed)
        m.ensure_optimizer()
        workspace(P * K)
        if h.get('crop_store', CROP_STORE_DEFAULT):
            inputs = TripletInputs(m.ctx, m.dev, self.image_size, labels, tr_gen.path, tr_gen.batch_size, store_budget(h, m.dev),
                                   self._loader_threads(), slots=max(3 * tr_gen.batch_size, P * K))
        else:
            inputs = TripletInputs(m.ctx, m.dev, self.image_size, labels, tr_gen.path, tr_gen.batch_size, 0, self._loader_threads(),
                                   tier=HOST)
        try:
            for e in range(epochs):
                batches = pk_batches(codes, P, K, rng)[:steps]
                drawn.append(batches)
                feed = inputs.crop_batches([[labels[r] for r in b] for b in batches])
                losses = [step(x, codes[b]).clone() for b, x in zip(batches, feed)]
                report(e, float(torch.cat(losses).double().mean().cpu()) if losses else float('nan'))
        finally:
            inputs.close()

    def _train_classes(self, tr_gen, ms, steps, epochs):
        """train() with hps['margin_softmax']: the batches of _train_pk (pk_batches, one generator seeded
        with pk_seed), every one through FidModel.train_on_classified_batch with the rows' subject codes as class labels,
        C = max code + 1.  The class kernel is read from face_identifier_classes.h5 when model_loading is set and the file holds
        this db's subject list, and initialised (ms_seed) otherwise; it is written back, with the subject list, after the last
        epoch.  Per epoch one line: the mean loss, the training accuracy (pred == label over the labelled rows) and the mean
        target cosine, summed on the device and read back once.  self.last_margin_softmax: the batches of every epoch, the class
        count, the last epoch's accuracy and mean cosine."""
        from .hdf5_lite import write_hdf5
        m, h = self.model, self.hps
        sids = list(tr_gen.db['subject_id'])
        codes = subject_codes(sids)
        C = int(codes.max()) + 1 if len(codes) else 0
        if C < 1:
            raise ValueError('fi_conf.hps.margin_softmax: the db holds no subject with a known identity')
        check_class_count(C)
        subjects = subject_list(sids, codes)
        kernel = self._saved_classes(subjects) if self.model_loading else None
        if kernel is None:
            m.init_classes(C, ms['seed'])
        else:
            m.set_classes(kernel)
        last = self.last_margin_softmax = dict(batches=[], classes=C, accuracy=None, cos_t=None)
        sums = torch.zeros(3, dtype=torch.float64, device=m.dev)      # this epoch's labelled rows, hits, sum of cos_t

        def step(x, row_codes):
            lab = torch.from_numpy(row_codes).to(m.dev)
            loss = m.train_on_classified_batch(x, lab, ms['kind'], ms['scale'], ms['margin'], h['lr'], h['beta_1'], h['beta_2'],
                                               h.get('decay', 0.0))
            sel = m.class_selection
            known = lab >= 0
            sums.add_(torch.stack([known.sum().double(), ((sel['pred'] == lab) & known).sum().double(),
                                   torch.where(known, sel['cos_t'], torch.zeros_like(sel['cos_t'])).sum()]))
            return loss

        def report(e, mean):
            n, hits, cs = (float(v) for v in sums.cpu())
            sums.zero_()
            acc, ct = (hits / n, cs / n) if n else (float('nan'), float('nan'))
            last.update(accuracy=acc, cos_t=ct)
            print('Epoch %d/%d - loss: %.4f - margin softmax (%s) accuracy: %.4f, target cosine: %.4f' % (e + 1, epochs, mean, ms['kind'], acc, ct))
        self._train_labelled(tr_gen, ms['P'], ms['K'], ms['pk_seed'], steps, epochs, last['batches'], m._cls_workspace, step, report)
        write_hdf5(self.CLASSES_PATH, {'/class_kernel': m.class_kernel.cpu().numpy(), '/subject_ids': subjects})

    def _saved_classes(self, subjects):
        """The class kernel of face_identifier_classes.h5 when the file is there and holds this subject list, else None."""
        from .hdf5_lite import is_hdf5, read_hdf5
        if not os.path.exists(self.CLASSES_PATH) or not is_hdf5(self.CLASSES_PATH):
            return None
        data, _ = read_hdf5(self.CLASSES_PATH)
        kernel, ids = data.get('/class_kernel'), data.get('/subject_ids')
        if kernel is None or ids is None or np.asarray(kernel).shape != (len(subjects), DENSE1_DIM):
            return None
        ids = np.asarray(ids)
        if ids.shape != subjects.shape or ids.dtype.kind != subjects.dtype.kind or not np.array_equal(ids, subjects):
            return None
        return np.asarray(kernel, np.float32)

    # ------------------------------------------------------------------ triplet mining
    def _sequence(self):
        if self.conf['resource_type'] == RESOURCE_TYPE_UCCS:
            return self.TrainingSequence
        if self.conf['resource_type'] == RESOURCE_TYPE_VGGFACE2:
            return self.TrainingSequenceVGGFace2
        raise ValueError('resource type is not valid.')

    def _db_ids(self, tr_gen, inputs):
        """Facial IDs (n, 64), on the device, of every row of the sequence's db in list(tr_gen.db.index) order, inference mode, in
        chunks of at most Engine.max_infer_batch(S) crops.  A resident TripletInputs: gathered from its store (nothing is decoded
        again); otherwise decoded through _extract_from_store, or on the host when hps['crop_store'] is off."""
        from .crop_store import RESIDENT
        from .engine import Engine
        m, labels = self.model, list(tr_gen.db.index)
        n, step = len(labels), max(1, Engine.max_infer_batch(self.image_size))
        if inputs is not None and inputs.tier == RESIDENT:
            ids = [m.extract_device(inputs.store.gather([inputs.slot_of[label] for label in labels[i:i + step]]))
                   for i in range(0, n, step)]
        elif self.hps.get('crop_store', CROP_STORE_DEFAULT):
            ids = self._extract_from_store([tr_gen.path(label) for label in labels], step)
        else:
            ids = [m.extract_device(np.asarray([_imread(tr_gen.path(label)) for label in labels[i:i + step]]))
                   for i in range(0, n, step)]
        return torch.cat(ids)

    def mine_triplets(self, drop_easy=False, tr_gen=None, inputs=None):
        """Every (anchor, positive) pair of the sequence's triplet list, in the list's order, with the negative the current model
        asks for (fv_fid_mine_negatives with hps['triplet_mining'], 'semi_hard' where that is off; margin TRIPLET_MARGIN) instead
        of the reference's random one -> (rows, kinds): the (anchor, positive, negative) label triples of mined_rows and, aligned
        with them, each row's kind (KIND_*).  Pairs whose anchor has subject -1 are left out: unknown identities are not known to
        be one person.  self.last_mining holds the number of pairs of each kind before anything was dropped, and the wall time.
        tr_gen / inputs: train()'s sequence and TripletInputs; alone, the sequence is built here (the pickle is read when there
        is one, written otherwise) and the crops are decoded through a store of their own."""
        t0 = time.time()
        if tr_gen is None:
            sequence = self._sequence()
            tr_gen = sequence(self.raw_data_path, dict(self.hps), self.nn_arch, load_flag=os.path.exists(sequence.PICKLE_FILE))
        m = self.model
        labels = list(tr_gen.db.index)
        slot_of = {label: k for k, label in enumerate(labels)}
        subjects = subject_codes(list(tr_gen.db['subject_id']))
        pairs = [(t[0], t[1]) for t in tr_gen.img_triplet_pairs if subjects[slot_of[t[0]]] >= 0]
        ids = self._db_ids(tr_gen, inputs)
        slots = np.asarray([(slot_of[a], slot_of[p]) for a, p in pairs], np.int64).reshape(-1, 2)
        anchors, pos_off, positives, order = triplet_groups(slots, sort=True)
        neg, kind, _dap, _dan = fid_mine_negatives(m.ctx, ids, torch.from_numpy(subjects).to(m.dev), anchors, pos_off, positives,
                                                   TRIPLET_MARGIN, self.mining or 'semi_hard')
        neg_of, kind_of = np.empty(len(pairs), np.int32), np.empty(len(pairs), np.int32)
        neg_of[order], kind_of[order] = neg.cpu().numpy(), kind.cpu().numpy()
        rows = mined_rows(pairs, neg_of, kind_of, labels, drop_easy)
        kinds = kind_of[(kind_of != KIND_NONE) & ~(bool(drop_easy) & (kind_of == KIND_EASY))]
        self.last_mining = dict(counts=[int((kind_of == k).sum()) for k in range(4)], seconds=time.time() - t0)
        return rows, kinds

    # ------------------------------------------------------------------ facial-ID database (fi.py:645-770)
    def _extract_db(self):
        """Facial IDs of every face crop of the subject db (subject -1 skipped), in groupby order -> (names, subject ids, IDs).
        The crops go through the extractor in chunks of at most Engine.max_infer_batch(S) images, mixed across subjects: an
        image's ID does not depend on the rest of its batch (fv_fid_extract), so this equals the reference's one predict per
        subject."""
        import pandas as pd
        db_file, faces_dir, _h5, _pk = db_files(self.conf['resource_type'])
        db = pd.read_csv(db_file).iloc[:, 1:]
        names, sids = [], []
        for subject_id, df in db.groupby('subject_id'):
            if subject_id == -1:
                continue
            for ff in list(df.iloc[:, 1]):
                names.append(ff); sids.append(subject_id)
        ids = [d.cpu().numpy() for d in self._extract_faces(faces_dir, names)]
        ids = np.concatenate(ids) if ids else np.zeros((0, DENSE1_DIM), np.float32)
        self._db_cache = (names, sids, ids)
        return names, sids, ids

    def _extract_faces(self, faces_dir, names):
        """Facial IDs of the crop files `names` of faces_dir, in that order -> device tensors, one per chunk of at most
        Engine.max_infer_batch(S) crops: through the crop store when hps['crop_store'] is on, decoded on the host otherwise."""
        from .engine import Engine
        step = max(1, Engine.max_infer_batch(self.image_size))
        paths = [os.path.join(self.raw_data_path, faces_dir, ff) for ff in names]
        if self.hps.get('crop_store', CROP_STORE_DEFAULT) and names:
            return self._extract_from_store(paths, step)
        return [self.fid_extractor.predict_device(np.asarray([_imread(f) for f in paths[i:i + step]]))
                for i in range(0, len(names), step)]

    def _extract_from_store(self, paths, step):
        """Facial IDs (device tensors, one per chunk of at most `step` crops) of the crop files `paths` through a CropStore:
        decoded on the loader pool; a db within the budget (crop_store.store_budget, taken once the extraction workspace exists)
        is loaded once and gathered chunk by chunk, a larger one is loaded chunk by chunk into two stores that alternate."""
        from concurrent.futures import ThreadPoolExecutor
        from .crop_store import RESIDENT, CropStore, plan_store, store_budget
        from .postproc import PinnedRing
        m, S, n = self.model, self.image_size, len(paths)
        m._workspace(min(step, n), S, False)
        ids = []
        with ThreadPoolExecutor(max_workers=self._loader_threads()) as pool:
            if plan_store(n, S, store_budget(self.hps, m.dev)) == RESIDENT:
                store = CropStore(m.ctx, n, S, m.dev)
                store.load(paths, list(range(n)), pool)
                for i in range(0, n, step):
                    ids.append(m.extract_device(store.gather(range(i, min(i + step, n)))))
            else:
                ring = PinnedRing(2)
                stores = [CropStore(m.ctx, min(step, n), S, m.dev, ring) for _ in range(2)]
                for k, i in enumerate(range(0, n, step)):
                    part = paths[i:i + step]
                    stores[k % 2].load(part, list(range(len(part))), pool)
                    ids.append(m.extract_device(stores[k % 2].gather(range(len(part)))))
        return ids

    def make_facial_ids_db(self):
        """fi.py:645-700: subject_facial_ids.h5 (vggface2: subject_facial_vggface2_ids.h5), one dataset per face file."""
        names, sids, ids = self._extract_db()
        write_facial_ids_h5(db_files(self.conf['resource_type'])[2], names, ids, sids)

    def register_facial_ids(self):
        """fi.py:702-770: every subject's mean facial ID, pickled as {subject_id: vector} (keys in groupby order) to
        ref_facial_id_db.pickle (vggface2: ref_facial_id_vggface2_db.pickle).  Right after make_facial_ids_db in the same process
        the IDs it extracted are reused."""
        names, sids, ids = self._db_cache if getattr(self, '_db_cache', None) is not None else self._extract_db()
        self._db_cache = None
        reg, order = {}, []
        for k, sid in enumerate(sids):
            if sid not in reg:
                reg[sid] = []; order.append(sid)
            reg[sid].append(ids[k])
        db = {sid: subject_mean(np.asarray(reg[sid])) for sid in order}
        with open(db_files(self.conf['resource_type'])[3], 'wb') as f:
            pickle.dump(db, f)

    # ------------------------------------------------------------------ unlabelled faces
    def cluster_unknown(self, eps=None, min_pts=None):
        """Group the faces nobody labelled: every crop of the subject db with subject_id -1, in db order, goes through the
        extractor (the path _extract_db takes) and fv_fid_cluster (eps, min_pts: hps['cluster']'s, or its defaults -- sim_th and
        3 -- where the key is off), with one copy back.  Writes subject_clusters.csv (vggface2: subject_clusters_vggface2.csv;
        cluster_csv_text) and returns dict(names, ids, labels, core, n_nbr, via, n_clusters): lists and NumPy arrays.  A db
        without such crops writes the header alone."""
        import pandas as pd
        conf = self.cluster if self.cluster is not None else cluster_conf(dict(self.hps, cluster=True))
        eps = conf['eps'] if eps is None else eps
        min_pts = conf['min_pts'] if min_pts is None else min_pts
        resource_type = self.conf['resource_type']
        db_file, faces_dir, _h5, _pk = db_files(resource_type)
        db = pd.read_csv(db_file).iloc[:, 1:]
        names = [str(ff) for ff in db.iloc[:, 1][db['subject_id'] == -1]]
        m = self.model
        if len(names) > CLUSTER_MAX_ROWS:
            raise ValueError('cluster_unknown: the db holds %d crops with subject_id -1, one fv_fid_cluster call takes %d'
                             % (len(names), CLUSTER_MAX_ROWS))
        chunks = self._extract_faces(faces_dir, names)
        ids = torch.cat(chunks) if chunks else torch.zeros((0, DENSE1_DIM), dtype=torch.float32, device=m.dev)
        out = fid_cluster(m.ctx, ids, eps, min_pts)
        # one copy back: the IDs and the five outputs as bytes of one buffer
        parts = [ids, out['labels'], out['via'], out['n_nbr'], out['n_clusters'], out['core']]
        host = torch.cat([t.contiguous().view(-1).view(torch.uint8) for t in parts]).cpu().numpy()
        cut = np.cumsum([0] + [t.numel() * t.element_size() for t in parts])
        ids_h, labels, via, n_nbr, n_clusters, core = [host[a:b].view(dt).copy() for a, b, dt in zip(
            cut[:-1], cut[1:], (np.float32, np.int32, np.int32, np.int32, np.int32, np.uint8))]
        with open(cluster_files(resource_type), 'w') as f:
            f.write(cluster_csv_text(names, labels, core, n_nbr, via))
        return dict(names=names, ids=ids_h.reshape(-1, DENSE1_DIM), labels=labels, core=core, n_nbr=n_nbr, via=via,
                    n_clusters=int(n_clusters[0]))

    def register_clusters(self, result, first_id=None):
        """One new subject per cluster of cluster_unknown's result, appended to the registry pickle register_facial_ids writes
        (an absent file is an empty registry): cluster c becomes subject first_id + c (first_id: 1 + the largest registered id, 0
        for an empty registry) with subject_mean of its members' facial IDs.  Existing entries and their order are kept.
        ValueError, before the file is written, when a new id is registered already.  -> the new ids."""
        path = db_files(self.conf['resource_type'])[3]
        db = {}
        if os.path.exists(path):
            with open(path, 'rb') as f:
                db = pickle.load(f)
        C = int(result['n_clusters'])
        if first_id is None:
            first_id = 1 + max(int(k) for k in db) if db else 0
        new_ids = [int(first_id) + c for c in range(C)]
        taken = sorted(set(new_ids) & set(int(k) for k in db))
        if taken:
            raise ValueError('register_clusters: subject id %s is registered already (first_id %d, %d clusters)'
                             % (', '.join(map(str, taken)), int(first_id), C))
        labels, ids = np.asarray(result['labels']), np.asarray(result['ids'])
        out = dict(db)
        for c, sid in enumerate(new_ids):
            out[sid] = subject_mean(ids[labels == c])
        with open(path, 'wb') as f:
            pickle.dump(out, f)
        return new_ids

    # ------------------------------------------------------------------ evaluate / test (fi.py:772-992, 994-1153)
    def _identify_files(self, on_batch):
        """The loop test() and evaluate() share.  Detect faces in every <test_path>/*.jpg (sorted) through the detector's
        pipelined loop (FaceDetector._detect_files), which runs the frames in batches; per batch the face crops are cut and
        letterboxed on the device from the batch's decoded images (fv_letterbox_crops), extracted in chunks of at most
        Engine.max_infer_batch(S) (fv_fid_extract) and matched against ref_facial_id_db.pickle in one launch (fv_fid_match);
        the `name,subject_id,xmin,ymin,w,h,score` rows go to output_file_path -- rows, order and text as the reference's
        per-crop loop -- and every box that got a row has its subject_id set (fi.py:928-929; the others keep -1).
        on_batch(group, images), if given, is then called with the batch's items (file name, None, boxes, (images, index)) and
        its decoded images (device uint8 buffer, offsets, hw), while the detector's generator is suspended -- its thread pool
        (self.fd._pool) is alive.  The caller has checked the image sizes."""
        from .engine import Engine
        test_path = self.conf['test_path']
        out_path = self.conf['output_file_path']
        with open('ref_facial_id_db.pickle', 'rb') as f:
            db = pickle.load(f)
        subject_ids = list(db.keys())
        if not subject_ids:
            raise ValueError('ref_facial_id_db.pickle holds no registered facial IDs')
        m = self.model
        registry = torch.from_numpy(np.asarray([db[k] for k in subject_ids], np.float32)).to(m.dev)   # uploaded once
        sim_th = self.hps['sim_th']
        S = self.image_size
        step = max(1, Engine.max_infer_batch(S))
        files = sorted(glob.glob(os.path.join(test_path, '*.jpg')))

        def flush(group, f):
            images = group[0][3][0]
            hw = images[2]
            rects = [crop_rects(it[2], hw[2 * it[3][1]], hw[2 * it[3][1] + 1], S) for it in group]
            crops = [(it[3][1],) + r for it, rs in zip(group, rects) for r in rs if r is not None]
            ids = []
            for c0 in range(0, len(crops), step):
                x = letterbox_crops(m.ctx, images, crops[c0:c0 + step], S)
                ids.append(m.extract_device(x))
            if crops:
                bi, bd = fid_match(m.ctx, torch.cat(ids), registry)
                bi, bd = bi.cpu().numpy(), bd.cpu().numpy()
            k = 0
            for it, rs in zip(group, rects):
                idx = np.full(len(rs), -1, np.int64); dist = np.full(len(rs), np.inf)
                for j, r in enumerate(rs):
                    if r is not None:
                        idx[j], dist[j] = bi[k], bd[k]; k += 1
                f.write(identification_rows(it[0], it[2], rs, idx, dist, subject_ids, sim_th))
                for j in matched_boxes(rs, dist, sim_th):
                    it[2][j].subject_id = subject_ids[int(idx[j])]
            if on_batch is not None:
                on_batch(group, images)

        with open(out_path, 'w') as f:
            group = []
            for item in self.fd._detect_files(files, need_raw=False, _with_images=True):
                if group and group[0][3][0] is not item[3][0]:
                    flush(group, f); group = []
                group.append(item)
                if item[0] == files[-1]:       # the last batch is flushed before the generator ends and takes its pool with it
                    flush(group, f); group = []

    def _check_fd_size(self):
        fd_size = int(self._full_conf['fd_conf']['nn_arch']['image_size'])
        if fd_size != self.image_size:
            raise ValueError('fd_conf.nn_arch.image_size (%d) must equal fi_conf.nn_arch.image_size (%d): the reference letterboxes '
                             'the frames with the identifier\'s size for the detector' % (fd_size, self.image_size))

    def test(self):
        """Detect faces in every <test_path>/*.jpg (sorted), identify each against ref_facial_id_db.pickle and write
        `name,subject_id,xmin,ymin,w,h,score` rows to output_file_path (_identify_files)."""
        self._check_fd_size()
        self._identify_files(None)

    def evaluate(self, device_encode=None):
        """fi.py:772-992: test()'s solution csv (the same rows, byte for byte), and under <test_path>/results_fi/ (emptied first)
        an annotated copy `<name>_detected.jpg` of every frame that has rows in <test_path>/validation.csv of which at least one
        survives ground_truth_boxes' filter, and at least one detection: ground truth in red, then the detections in green, each
        box labelled `score, class score, subject id` (draw_boxes_v3; -1 where no row was written for the box).
        The frames are not decoded a second time: per batch, once the crops are cut and extracted, ONE fv_draw_prims_u8 call
        draws every frame's boxes into the batch's decoded images on the device (annotate.annotation_prims), one device-to-host
        copy brings the drawn frames into a pinned slot, and the detector's thread pool encodes and writes them with Pillow
        while the next batch runs.  device_encode (None: hps['device_encode'], on where that is absent): the drawn frames are
        encoded on the device (jpeg.encode_batch: the same bytes Pillow writes), only the files cross to the host and the pool
        just writes them; a frame taller or wider than 65535 pixels still takes the Pillow path.
        Single process: multi_gpu is ignored, as in test().
        main() does not dispatch fi_conf.mode 'evaluate' yet: call this method."""
        import pandas as pd
        from concurrent.futures import wait
        from .postproc import PinnedRing
        self._check_fd_size()
        if device_encode is None:
            device_encode = bool(self.hps.get('device_encode', DEVICE_ENCODE_DEFAULT))
        res_dir = os.path.join(self.conf['test_path'], 'results_fi')
        if os.path.isdir(res_dir):
            shutil.rmtree(res_dir)
        os.mkdir(res_dir)
        gt_df = pd.read_csv(os.path.join(self.conf['test_path'], 'validation.csv'))
        groups = {k: v for k, v in gt_df.groupby('FILE')}
        font = _font()
        m = self.model
        ring = PinnedRing(2)
        saves = [[], []]                           # per pinned slot: the writes still reading it
        state = {'takes': 0, 'all': []}

        def annotate(group, images):
            dbuf, offs, hw = images
            prims, frames = [], []
            for name, _raw, boxes, (_imgs, i) in group:
                base = name.split('\\')[-1] if platform.system() == 'Windows' else name.split('/')[-1]
                df = groups.get(base)
                gt_boxes = ground_truth_boxes(df) if df is not None else []
                if len(gt_boxes) == 0 or len(boxes) == 0:
                    continue
                prims += annotation_prims(i, gt_boxes, (255, 0, 0), font) + annotation_prims(i, boxes, (0, 255, 0), font)
                frames.append((i, os.path.join(res_dir, base[:-4] + '_detected' + base[-4:])))
            if not frames:
                return
            prims, masks = pack_masks(prims)
            draw_prims_u8(m.ctx, images, prims, torch.from_numpy(masks).to(dbuf.device) if masks.size else None)
            on_dev = [f for f in frames if encode_on_device(device_encode, hw[2 * f[0]], hw[2 * f[0] + 1])]
            if on_dev:
                from . import jpeg
                slot = state['takes'] % 2
                state['takes'] += 1
                wait(saves[slot])
                files = jpeg.encode_batch(m.ctx, dbuf, [offs[i] for i, _ in on_dev],
                                          [v for i, _ in on_dev for v in hw[2 * i:2 * i + 2]], dbuf.device, pinned=ring.take)
                saves[slot] = [self.fd._pool.submit(write_bytes, data, path) for data, (_, path) in zip(files, on_dev)]
                state['all'] += saves[slot]
                frames = [f for f in frames if f not in on_dev]
                if not frames:
                    return
            lo = min(offs[i] for i, _ in frames)
            hi = max(offs[i] + hw[2 * i] * hw[2 * i + 1] * 3 for i, _ in frames)
            slot = state['takes'] % 2
            state['takes'] += 1
            wait(saves[slot])                      # the writes of two copies ago have let go of the slot
            host = ring.take(hi - lo)
            host.copy_(dbuf[lo:hi], non_blocking=True)
            torch.cuda.current_stream(dbuf.device).synchronize()
            view = host.numpy()
            saves[slot] = [self.fd._pool.submit(save_frame, view[offs[i] - lo:offs[i] - lo + hw[2 * i] * hw[2 * i + 1] * 3]
                                                .reshape(hw[2 * i], hw[2 * i + 1], 3), path) for i, path in frames]
            state['all'] += saves[slot]

        self._identify_files(annotate)
        wait(state['all'])
        for w in state['all']:
            w.result()


def main():
    """Reads ./face_vijnana_yolov3.json (Windows: _win) and dispatches on fi_conf.mode (fi.py:1715-1760):
      data    create_db_fi: the face crops and the subject db of fi_conf.resource_type (no model is built); a configuration
              that names neither 'uccs' nor 'vggface2' is refused like a mode that is not implemented;
      train   trains and saves face_identifier.h5, then builds the facial-ID database (make_facial_ids_db, register_facial_ids),
              as fi.py:1734-1743 does.  With fi_conf.multi_gpu and num_gpus > 1 this process starts num_gpus ranks of itself
              (parallel.launch_ranks) before any GPU call and exits with their code; the ranks train data-parallel, then rank 0
              alone builds the database (the others return after train());
      fid_db  make_facial_ids_db, then register_facial_ids -- the reference leaves the second call commented out, but nothing else
              would register the IDs of a loaded model, and test() reads the registry;
      test    test() -> output_file_path;
      cluster cluster_unknown() -> subject_clusters.csv: the db's crops with subject_id -1 grouped by fv_fid_cluster (not in the
              reference), then register_clusters() when hps.cluster.register is true.
    'evaluate' is not implemented here; the other modes ignore multi_gpu."""
    name = 'face_vijnana_yolov3_win.json' if platform.system() == 'Windows' else 'face_vijnana_yolov3.json'
    with open(name, 'r') as f:
        conf = json.load(f)
    mode = conf['fi_conf']['mode']
    if mode not in ('data', 'train', 'fid_db', 'test', 'cluster'):
        raise NotImplementedError('fi_conf.mode %r is not implemented (available: data, train, fid_db, test, cluster)' % mode)
    if mode == 'data':                     # needs no model
        resource_type = conf['fi_conf'].get('resource_type')
        if resource_type not in (RESOURCE_TYPE_UCCS, RESOURCE_TYPE_VGGFACE2):
            raise NotImplementedError('fi_conf.mode \'data\' is not implemented for resource_type %r (available: %s, %s)'
                                      % (resource_type, RESOURCE_TYPE_UCCS, RESOURCE_TYPE_VGGFACE2))
        ts = time.time()
        create_db_fi(conf)
        print('Elasped time: {0:f}s'.format(time.time() - ts))
        return
    if mode == 'train':
        n = int(conf['fi_conf'].get('num_gpus', 1)) if conf['fi_conf'].get('multi_gpu') else 1
        refuse_mining_on_ranks(conf['fi_conf'].get('hps', {}), n)         # before a rank is started
        if n > 1 and 'WORLD_SIZE' not in os.environ:
            # multi_gpu_model(model, gpus=num_gpus) (fi.py:348-361) is one process driving num_gpus towers; here it is one process
            # per GPU, started from this one BEFORE it makes any GPU call -- the reference's command line stays what it was
            from .parallel import launch_ranks
            raise SystemExit(launch_ranks(n, ['-m', 'face_vijnana_yolov3_amd.face_identification']))
    fi =FaceIdentifier(conf)
    ts = time.time()
    if mode == 'train':
        fi.train()                         # ends the process group
        if conf['fi_conf'].get('multi_gpu') and int(os.environ.get('WORLD_SIZE', 1)) > 1 and int(os.environ.get('RANK', 0)) != 0:
            return                         # the database is rank 0's job
        fi.make_facial_ids_db()
        fi.register_facial_ids()
    elif mode == 'fid_db':
        fi.make_facial_ids_db()
        fi.register_facial_ids()
    elif mode == 'cluster':
        result = fi.cluster_unknown()
        if fi.cluster is not None and fi.cluster['register']:
            fi.register_clusters(result)
    else:
        fi.test()
    print('Elasped time: {0:f}s'.format(time.time() - ts))


if __name__ == '__main__':
    main()
