"""The arms of the voxel gathers and of the channels-last devoxelize that only an A/B switch reaches (csrc/voxel_gather.hip,
csrc/devoxelize.hip; the switches are keys of P2PB_EXPERIMENT, p2p_bridge_amd/_experiment.py), held to the same bits as the
arms production picks. The library reads a switch once per process, hence one child process per setting.

vox_onepass=1 (every voxel in one pass whatever the shape): at C = 35 vox_gather_cl_all_kernel<false> and
    vox_gather_cl_split_kernel<false>, which the default rule never picks (a channel count that is no multiple of 4 takes the
    occupied forms); at C = 64, N = 128, r = 8 the one-pass split kernel where the default takes the occupied one.
vox_onepass=0 (zero-fill + the occupied voxels only): at C = 16 / 12 / 64 vox_gather_cl_occ_kernel on 16-byte rows and
    vox_gather_cl_occ_split_kernel<true> at r^3 < 4 N.
devox_cl4=0: devox_cl_kernel (4-byte gathers, the write-back with clamped rows) at C % 64 == 0, where the default takes
    devox_cl4_kernel.

Voxelize: the first five VOX_SHAPES of test_fused_discipline_gpu.py with its planted crowded voxel, through
test_voxel_sort_and_gather itself (inside the poisoned arena: cnt, the fp32 grid and the split grid bit-equal to
oracle.cpu_ops.avg_voxelize_forward and to conv3d_presplit(fp32 grid), the split grid's padded channels all-zero bits).
Devoxelize: compute_devox() of test_gather_batching_gpu.py at C = 64 and 128 (both r, all four N, affine and point branch on
and off: 64 outputs) against the devox/ digests of tests/golden/gather_tails.npz, which the 16-byte form wrote."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = r"""
import os, sys
root = %r
sys.path[:0] = [root, os.path.join(root, "tests")]
import numpy as np
import torch
from oracle.poison_arena import PoisonArena
from p2p_bridge_amd import fused
import test_fused_discipline_gpu as fd
import test_gather_batching_gpu as gb

for shape in fd.VOX_SHAPES[:5]:
    with PoisonArena("cuda", fd.ARENA_BYTES) as arena:
        fd.test_voxel_sort_and_gather(arena, fused, *shape)
print("VOXELIZE-OK")
if "devox" in sys.argv[1:]:
    gb.DV_C = [64, 128]
    got = gb.compute_devox()
    with np.load(gb.GOLDEN_FILE) as z:
        want = {k: z[k] for k in z.files if k.startswith("devox/") and k.split("/")[1].split("_")[2] in ("c64", "c128")}
    assert sorted(got) == sorted(want) and len(want) == len(gb.DV_R) * len(gb.DV_N) * 2 * 4, (len(got), len(want))
    bad = [k for k in sorted(want) if not np.array_equal(got[k], want[k])]
    assert not bad, "%%d of %%d outputs of the 4-byte form differ from the recorded bits, first: %%s" %% (len(bad), len(want), bad[:6])
    print("DEVOXELIZE-OK")
""" % ROOT


@pytest.mark.parametrize("experiment,devox", [("vox_onepass=1;devox_cl4=0", True), ("vox_onepass=0", False)])
def test_switch_only_arms(experiment, devox):
    env = dict(os.environ, P2PB_EXPERIMENT=experiment)
    r = subprocess.run([sys.executable, "-c", CODE] + (["devox"] if devox else []), env=env, capture_output=True, text=True,
                       timeout=300)
    ok = r.returncode == 0 and "VOXELIZE-OK" in r.stdout and (not devox or "DEVOXELIZE-OK" in r.stdout)
    assert ok, (r.stdout[-1500:], r.stderr[-3000:])
