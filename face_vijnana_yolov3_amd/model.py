"""What the three device models (Engine, Yolov3, FidModel) share on the host: the flat parameter / BN-state / Adam vectors
(torch-ROCm tensors used as plain storage), the synthetic initialisation, the workspace cache, the training-call plumbing, the
split of an inference batch beyond one buffer descriptor, and the checkpoint files.  Each model adds its C entry points."""
import ctypes

import numpy as np
import torch

from . import ops, weights
from ._lib import BUCKET_FN, FvError, LayerDesc, lib, ptr
from .weights import NUM_BASE_LAYERS

_NO_BUCKET = ctypes.cast(None, BUCKET_FN)


def layer_table(count, layer):
    """List of dicts mirroring fv_layer_desc, read through count() and layer(i, desc*) (works without a GPU)."""
    out = []
    for i in range(count()):
        d = LayerDesc()
        assert layer(i, ctypes.byref(d)) == 0
        out.append({f: getattr(d, f) for f, _ in LayerDesc._fields_})
    return out


class Model(object):
    BN_UPDATES_PER_STEP = 1         # BN moving-statistics updates one training call applies

    def __init__(self, ctx, layers, n_params, n_state):
        self.ctx = ctx
        self.dev = torch.device('cuda', ctx.device)
        self.layers = layers
        self.n_params = int(n_params)
        self.n_state = int(n_state)
        self.params = torch.zeros(self.n_params, dtype=torch.float32, device=self.dev)
        self.state = torch.zeros(self.n_state, dtype=torch.float32, device=self.dev)
        self.grads = self.m = self.v = None
        self.iterations = 0
        # Keras 2.2.4 / TF 1.x update of the BN moving statistics (zero-debiased, fv_set_bn_zero_debias_step) instead of the plain
        # EMA; bn_updates counts the updates of THIS object (TF keeps the step in a graph variable that load_model rebuilds)
        self.bn_zero_debias = False
        self.bn_updates = 0
        self._ws = {}
        self._loss = torch.zeros(1, dtype=torch.float32, device=self.dev)
        self._bucket_cb = None

    # ------------------------------------------------------------------ parameters
    def set_params(self, params, state):
        params = torch.as_tensor(params, dtype=torch.float32).reshape(-1)
        state = torch.as_tensor(state, dtype=torch.float32).reshape(-1)
        assert params.numel() == self.n_params and state.numel() == self.n_state
        self.params.copy_(params)
        self.state.copy_(state)

    def set_base(self, params, state):
        """Copy the 52 base layers and their BN statistics: the prefix of the flat vectors, the same in every model's layout (the
        detector's vectors, a base file's)."""
        d = self.layers[NUM_BASE_LAYERS - 1]
        n_p, n_s = d['beta_off'] + d['cout'], d['var_off'] + d['cout']
        self.params[:n_p].copy_(torch.as_tensor(params, dtype=torch.float32).reshape(-1)[:n_p])
        self.state[:n_s].copy_(torch.as_tensor(state, dtype=torch.float32).reshape(-1)[:n_s])

    def init_synthetic(self, seed=7):
        """Random-init weights of the SURVEY 8d config-2 shape (no pretrained file offline), layer by layer: BN layers' kernels
        ~ N(0, 2/fan_in), gamma 1, beta 0, moving mean 0 / var 1; the others glorot-uniform with zero bias.  Everything outside
        self.layers is zeroed."""
        g = torch.Generator(device='cpu').manual_seed(seed)
        p = torch.zeros(self.n_params, dtype=torch.float32)
        s = torch.zeros(self.n_state, dtype=torch.float32)
        for d in self.layers:
            k, cin, cout = d['ksize'], d['cin'], d['cout']
            n = cout * k * k * cin
            if d['has_bn']:
                p[d['w_off']:d['w_off'] + n] = torch.randn(n, generator=g) * float(np.sqrt(2.0 / (k * k * cin)))
                p[d['gamma_off']:d['gamma_off'] + cout] = 1.0
                s[d['var_off']:d['var_off'] + cout] = 1.0
            else:
                lim = float(np.sqrt(6.0 / (k * k * cin + k * k * cout)))
                p[d['w_off']:d['w_off'] + n] = (torch.rand(n, generator=g) * 2 - 1) * lim
        self.set_params(p, s)

    # ------------------------------------------------------------------ workspaces
    def _workspace(self, batch, image_size, training):
        """Device workspace of one call (self._workspace_bytes); one is kept per mode (inference / training).  It is allocated
        uninitialised and reused call after call: the library ignores its contents on entry, and writes nothing outside
        [workspace, workspace + bytes)."""
        key = (batch, image_size, bool(training))
        if key not in self._ws:
            n = int(self._workspace_bytes(batch, image_size, 1 if training else 0))
            if n == 0:
                raise FvError('unsupported batch/image_size %r' % (key,))
            self._ws = {k: v for k, v in self._ws.items() if k[2] != bool(training)}
            self._ws[key] = torch.empty(n, dtype=torch.uint8, device=self.dev)
        return self._ws[key]

    def _train_tensor(self, batch, image_size, layer, code):
        """Flat float32 view of a tensor the last training call kept in its workspace (self._workspace_tensor; code 0 z, 1 a,
        2 mean, 3 invstd, 4 scale, 5 shift)."""
        off, cnt = ctypes.c_size_t(0), ctypes.c_int64(0)
        if self._workspace_tensor(batch, image_size, layer, code, ctypes.byref(off), ctypes.byref(cnt)) != 0:
            raise FvError('no kept tensor %d of layer %d at batch %d, image size %d' % (code, layer, batch, image_size))
        ws = self._workspace(batch, image_size, True)
        return ws[off.value:off.value + 4 * cnt.value].view(torch.float32)

    def leaky_slopes_taken(self, batch, image_size):
        """Per BN layer, a bool tensor [B][H][W][C]: True where the last train step took the positive LeakyReLU branch, i.e.
        fl(fl(z*scale)+shift) > 0 -- the decision every kernel of the step makes (the library is built with -ffp-contract=off)."""
        out = []
        for l, d in enumerate(self.layers):
            if d['has_bn']:
                z, scale, shift = (self._train_tensor(batch, image_size, l, code) for code in (0, 4, 5))
                g = image_size // d['out_div']
                out.append((z.view(batch, g, g, d['cout']) * scale + shift) > 0)
        return out

    # ------------------------------------------------------------------ inference
    @staticmethod
    def max_infer_batch(image_size):
        """Largest batch one inference call takes at this image size: the kernels address a tensor through one buffer descriptor
        (2 GiB, 2^29 floats) and the largest activation, the first layer's batch x S x S x 32 output, must stay below 2^29."""
        return ((1 << 29) - 1) // (32 * int(image_size) * int(image_size))

    def _in_parts(self, forward, x, *args, image_size=None):
        """forward(x, *args) for images x (B,S,S,3).  Inference is per image (moving statistics): a batch beyond what one call
        addresses runs in parts of a multiple of 8 images, and the outputs (a tensor, a pair or a list) are concatenated.
        image_size: the side of the images the call works on when x does not hold them (ReconModel: x are facial IDs)."""
        B = x.shape[0]
        cap = self.max_infer_batch(x.shape[1] if image_size is None else image_size)
        if not B > cap >= 1:
            return forward(x, *args)
        step = cap // 8 * 8 if cap >= 8 else cap
        parts = [forward(x[i:i + step], *args) for i in range(0, B, step)]
        if torch.is_tensor(parts[0]):
            return torch.cat(parts)
        return type(parts[0])(torch.cat(outs) for outs in zip(*parts))

    # ------------------------------------------------------------------ training
    def ensure_optimizer(self):
        if self.grads is None:
            self.grads = torch.zeros_like(self.params)
            self.m = torch.zeros_like(self.params)
            self.v = torch.zeros_like(self.params)

    def _bucket_fn(self, on_bucket):
        """-> (BUCKET_FN for a training call, list that receives the first exception of on_bucket).  on_bucket(offset, count) is
        called as gradient ranges complete.  A ctypes callback prints and swallows an exception: _train_call re-raises the first
        one after the call, and later ranges are not forwarded.  The BUCKET_FN is kept alive in self._bucket_cb."""
        errors = []
        if on_bucket is None:
            self._bucket_cb = _NO_BUCKET
            return _NO_BUCKET, errors

        def cb(user, off, cnt):
            if errors:
                return
            try:
                on_bucket(int(off), int(cnt))
            except BaseException as e:   # noqa: B902
                errors.append(e)
        self._bucket_cb = BUCKET_FN(cb)
        return self._bucket_cb, errors

    def _train_call(self, name, *args, errors=(), bn_updates=None):
        """lib().name(handle, params, state, *args) with the zero-debias step of this call set before it; bn_updates advances by
        BN_UPDATES_PER_STEP (bn_updates: by that many instead -- a step over fewer towers).  Returns the loss, a 1-element CUDA
        tensor (no host sync)."""
        self.ctx.set_bn_zero_debias_step(self.bn_updates + 1 if self.bn_zero_debias else 0)
        rc = getattr(lib(), name)(self.ctx.handle, ptr(self.params), ptr(self.state), *args)
        self.ctx.check(rc, name)
        if errors:
            raise errors[0]
        self.bn_updates += self.BN_UPDATES_PER_STEP if bn_updates is None else bn_updates
        return self._loss

    def adam_step(self, lr, beta_1, beta_2, decay=0.0, eps=1e-7):
        ops.adam_step(self.ctx, self.params, self.grads, self.m, self.v, self.iterations, lr, beta_1, beta_2, eps, decay)
        self.iterations += 1

    # ------------------------------------------------------------------ checkpoints
    def _save(self, path, nested, **extras):
        """`*.h5`: _save_h5; any other extension: the plain .npz of rounds 1-2 (params, state, iterations, extras, Adam m / v)."""
        if str(path).endswith('.h5'):
            return self._save_h5(path, nested, **extras)
        d = dict(params=self.params.cpu().numpy(), state=self.state.cpu().numpy(), iterations=np.int64(self.iterations), **extras)
        if self.m is not None:
            d['m'] = self.m.cpu().numpy(); d['v'] = self.v.cpu().numpy()
        with open(path, 'wb') as f:
            np.savez(f, **d)

    def _save_h5(self, path, nested, more_groups=None, **extras):
        """A real HDF5 file in Keras' weight layout (weights.write_keras_h5 through the pure-Python hdf5_lite: `model.load_weights`
        of the reference's stack and h5py read it), with this build's step count, extras and Adam vectors under /fv.
        nested: the nested-Model layer that holds the BN layers, or None for one group per Keras layer."""
        fv = dict(iterations=np.int64(self.iterations), **extras)
        if self.m is not None:
            fv['adam_m'] = self.m.cpu().numpy(); fv['adam_v'] = self.v.cpu().numpy()
        weights.write_keras_h5(path, self.layers, self.params.cpu().numpy(), self.state.cpu().numpy(), nested=nested, extras=fv,
                               more_groups=more_groups)

    def _load(self, path, require_all=True, error=FvError, check=None, read_more=None):
        """HDF5 (a Keras weight / model file) or the .npz of rounds 1-2, told apart by the file signature.  check(path, fv) sees
        this build's entries first (/fv of an HDF5 file, the arrays of an .npz); read_more(path, datasets, params) fills what lies
        outside self.layers from an HDF5 file.  Both may raise before anything is changed.  require_all=False accepts a file that
        holds only some layers: the others keep their values.  Returns fv."""
        from .hdf5_lite import is_hdf5, read_hdf5
        if is_hdf5(path):
            datasets, _ = read_hdf5(path)
            fv = {k[len('/fv/'):]: v for k, v in datasets.items() if k.startswith('/fv/')}
            if check:
                check(path, fv)
            keep = () if require_all else (self.params.cpu().numpy(), self.state.cpu().numpy())
            p, st, found = weights.from_keras_datasets(datasets, self.layers, self.n_params, self.n_state, *keep)
            missing = sorted(set(weights.expected_keras_tensors(self.layers)) - set(found))
            if missing and require_all:
                raise error('%s lacks %d tensors of this model, e.g. %r' % (path, len(missing), missing[:3]))
            if read_more:
                read_more(path, datasets, p)
            m, v = fv.get('adam_m'), fv.get('adam_v')
        else:
            with open(path, 'rb') as f:
                fv = dict(np.load(f))
            if check:
                check(path, fv)
            p, st, m, v = fv['params'], fv['state'], fv.get('m'), fv.get('v')
        self.set_params(p, st)
        self.iterations = int(fv.get('iterations', 0))
        if m is not None and v is not None:
            self.ensure_optimizer()
            self.m.copy_(torch.as_tensor(np.asarray(m))); self.v.copy_(torch.as_tensor(np.asarray(v)))
        return fv
