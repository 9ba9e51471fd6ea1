"""tests/golden/gather_tails.npz: the outputs of the point-major gather / scatter-back kernels (group_stats, group_sub,
three_interp_add, devox_cl / devox_cl4 of csrc/devoxelize.hip with the folded tail, the one-pass split voxel gather of
csrc/voxel_gather.hip, the far-field constants, the SE3d gate) for the seeded inputs of tests/test_gather_batching_gpu.py, as the kernels BEFORE the batched-loads change wrote
them. Run once on the GPU with the library of that commit (P2PB_LIB_PATH, or the tree checked out there plus this file and
the test file); the test then holds every later form of these kernels to those bits. GroupNorm partials in full, large tensors as
SHA-256 digests (the test's docstring says why).     python tools/make_golden_gather_tails.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gather_batching_gpu as t  # noqa: E402

path = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN_FILE
out = t.compute_all()
again = t.compute_all()  # a recording that is not reproducible run to run would be no yardstick
assert all(np.array_equal(out[k], again[k]) for k in out), "outputs differ between two runs"
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")
