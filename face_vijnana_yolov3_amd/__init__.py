"""MI355X-native FaceDetector hot path (gfx950 HIP kernels behind a C ABI).

The product path never falls back to a CPU implementation: if libfv_hotpath.so is missing
or no MI355X is visible, calls raise."""
import os as _os

# The HIP runtime multiplexes a process's streams onto a fixed number of hardware queues (4 by default); the package leaves that
# number to the runtime.  fv_train_step overlaps its weight-gradients with the data-gradient chain on a low-priority side stream of
# its context; a context created AFTER an RCCL communicator has existed in the process (DataParallelTrainer, or bench.py's world-size-1
# rehearsal) can find its side stream sharing a hardware queue with the compute stream: the three-scale step ran 31.5 -> 43 ms and the
# 608 x 608 step 45.2 -> 51.7 ms, while contexts created before the communicator were unaffected.  Create contexts before
# communicators.

__version__ = '0.1.0'
