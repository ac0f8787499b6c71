"""Device engine behind FaceDetector: owns the flat parameter / optimiser / BN-state vectors
(torch-ROCm tensors used as plain storage) and drives the C-ABI hot path.

It plays the role of the compiled Keras `Model` in the reference (face_detection.py:341-382):
`predict` (fd.py:899), one `fit_generator` step (fd.py:621-627), `save`/`load` (fd.py:630, 337)."""
import torch

from . import model
from ._lib import Context, c_void_p, lib, ptr

HEAD_C = 6


def layer_table():
    """List of dicts mirroring fv_layer_desc (works without a GPU)."""
    return model.layer_table(lib().fv_num_layers, lib().fv_layer)


def fwd_flops_per_image(image_size=416):
    """2*MAC of the 52 base convs + the head at one image (49.050 GFLOP at 416)."""
    return sum(2 * (image_size // d['out_div']) ** 2 * d['ksize'] ** 2 * d['cin'] * d['cout'] for d in layer_table())


def train_flops_per_image(image_size=416):
    """forward + every weight-gradient + every data-gradient except conv_0's (146.85 GFLOP at 416)."""
    return 3 * fwd_flops_per_image(image_size) - 2 * image_size * image_size * 27 * 32


class Engine(model.Model):
    def __init__(self, device=0, stream=None):
        super(Engine, self).__init__(Context(device, stream), layer_table(), lib().fv_param_count(), lib().fv_state_count())

    def _workspace_bytes(self, batch, image_size, training):
        return lib().fv_workspace_bytes(batch, image_size, training)

    def _workspace_tensor(self, batch, image_size, layer, code, off, cnt):
        return lib().fv_train_workspace_tensor(batch, image_size, layer, code, off, cnt)

    def _as_input(self, x):
        x = torch.as_tensor(x)
        if x.dtype != torch.float32 or x.device != self.dev:
            x = x.to(device=self.dev, dtype=torch.float32)
        return x.contiguous()

    # ------------------------------------------------------------------ predict (fd.py:899)
    def predict_device(self, x):
        """x: (B,S,S,3) float in [0,1] -> (B,S/32,S/32,6) float32 CUDA tensor (stream-ordered)."""
        return self._in_parts(self._predict, self._as_input(x))

    def _predict(self, x):
        B, S = x.shape[0], x.shape[1]
        assert x.dim() == 4 and x.shape[2] == S and x.shape[3] == 3
        ws = self._workspace(B, S, False)
        y = torch.empty((B, S // 32, S // 32, HEAD_C), dtype=torch.float32, device=self.dev)
        rc = lib().fv_forward_infer(self.ctx.handle, ptr(self.params), ptr(self.state), ptr(x), B, S, ptr(ws), ws.numel(), ptr(y))
        self.ctx.check(rc, 'fv_forward_infer')
        return y

    def predict(self, x):
        return self.predict_device(x).cpu().numpy()

    def predict_base_device(self, x, with_head=False):
        """The base model alone (FaceDetector.YOLOV3Base, fd.py:384-600): x (B,S,S,3) -> the add_23 output (B,S/32,S/32,1024),
        float32 CUDA tensor; with_head=True also returns the head output of the same pass."""
        return self._in_parts(self._predict_base, self._as_input(x), with_head)

    def _predict_base(self, x, with_head):
        B, S = x.shape[0], x.shape[1]
        assert x.dim() == 4 and x.shape[2] == S and x.shape[3] == 3
        ws = self._workspace(B, S, False)
        feat = torch.empty((B, S // 32, S // 32, self.layers[-1]['cin']), dtype=torch.float32, device=self.dev)
        y = torch.empty((B, S // 32, S // 32, HEAD_C), dtype=torch.float32, device=self.dev) if with_head else None
        rc = lib().fv_forward_base(self.ctx.handle, ptr(self.params), ptr(self.state), ptr(x), B, S, ptr(ws), ws.numel(), ptr(feat),
                                   ptr(y) if with_head else c_void_p(None))
        self.ctx.check(rc, 'fv_forward_base')
        return (feat, y) if with_head else feat

    # ------------------------------------------------------------------ training
    def forward_backward(self, x, y_true, on_bucket=None, loss_weight=1.0):
        """fwd + mse + bwd; gradients land in self.grads; returns the loss as a 1-element CUDA
        tensor (no host sync).  on_bucket(offset, count) is called as gradient ranges complete.
        loss_weight: this slice's share n_r / N of a merged data-parallel batch (fv_train_step): scales the gradients, not the loss."""
        self.ensure_optimizer()
        x = self._as_input(x)
        y_true = self._as_input(y_true)
        B, S = x.shape[0], x.shape[1]
        assert y_true.shape == (B, S // 32, S // 32, HEAD_C), y_true.shape
        ws = self._workspace(B, S, True)
        cb, errors = self._bucket_fn(on_bucket)
        return self._train_call('fv_train_step', ptr(x), ptr(y_true), B, S, ptr(ws), ws.numel(), ptr(self.grads), ptr(self._loss),
                                float(loss_weight), cb, None, errors=errors)

    def train_tensor(self, batch, image_size, layer, which):
        """View into the training workspace after forward_backward (fv_train_workspace_tensor):
        which = 'z' | 'a' | 'mean' | 'invstd' | 'scale' | 'shift' of base layer `layer`."""
        code = {'z': 0, 'a': 1, 'mean': 2, 'invstd': 3, 'scale': 4, 'shift': 5}[which]
        t = self._train_tensor(batch, image_size, layer, code)
        if code <= 1:
            g = image_size // self.layers[layer]['out_div']
            t = t.view(batch, g, g, self.layers[layer]['cout'])
        return t

    def train_on_batch(self, x, y_true, lr, beta_1, beta_2, decay=0.0):
        loss = self.forward_backward(x, y_true)
        self.adam_step(lr, beta_1, beta_2, decay)
        return loss

    # ------------------------------------------------------------------ checkpoint (fd.py:630 model.save / fd.py:337 load_model)
    def save(self, path, nested='model_1'):
        """Weights + BN moving statistics + Adam state.  `*.h5` (the reference's MODEL_PATH / yolov3_base.h5 names) is written in
        Keras' weight layout (Model._save_h5); any other extension gets the plain .npz of rounds 1-2.  nested=None writes the
        one-group-per-layer layout of yolov3_base.h5."""
        self._save(path, nested)

    def load(self, path, require_all=True):
        """HDF5 (a Keras weight / model file: the reference's face_detector.h5 or yolov3_base.h5, or one written by save) or the
        .npz of rounds 1-2 -- told apart by the file signature.  require_all=False accepts a file that holds only some layers (the
        head keeps its current values)."""
        self._load(path, require_all)
