"""Drop-in for the reference's compiled extension module `pointops_cuda`
(third_party/openpoints/cpp/pointops/src/pointops_api.cpp:15-27; PO = that src directory): the 13 names with the pybind
argument order, on the gfx950 C-ABI library (csrc/pointops.hip, include/p2pb_hip.h). `p2p_bridge_amd.install_dropin()`
registers it under the reference's module name, so `openpoints/cpp/pointops/functions/pointops.py` runs unmodified.

A batch is one packed cloud xyz f32[n,3] with cumulative segment ends offset i32[b]; features are point-major f32[n,c].
The caller allocates and initialises every output and the kernels write into the caller's tensors on the current stream,
as in the reference. Sizes that the pybind signatures do not carry come from the tensors (b = offset.shape[0],
n = xyz.shape[0]). Where the reference trusts its arguments these raise RuntimeError: a tensor that is not on the GPU, a
wrong dtype, a non-contiguous tensor, a shape that disagrees with the integers passed, a non-zero return code.
`ballquery_cuda` returns 1 like the reference's, the others None.
"""
import types

import torch

from ._lib import P2PBError, ask, call, ptr, stream_ptr
from .pointnet2_batch_cuda import _pn2_check, avg_voxelize_backward, avg_voxelize_forward  # noqa: F401  (PO/voxelization/vox.cu is the file already served)

F32, I32 = torch.float32, torch.int32

_KNN_MAX = 100  # csrc/pointops.hip PO_KNN_MAX: the reference's per-thread arrays hold 100 entries and are overrun above


def _dim0(t, name):
    if not torch.is_tensor(t) or t.dim() < 1:
        raise RuntimeError(f"{name} must be a tensor with at least one dimension")
    return t.shape[0]


def _no_scatter_in_deterministic_mode(name):
    if ask("p2pb_get_deterministic"):
        raise P2PBError(f"{name}: no deterministic kernel (it accumulates with fp32 atomics, whose order is not fixed): run "
                        "this backward pass outside p2p_bridge_amd.deterministic()")


def knnquery_cuda(m, nsample, xyz, new_xyz, offset, new_offset, idx, dist2):
    """PO/knnquery/knnquery_cuda.cpp. -> idx i32[m,nsample] (global indices), dist2 f32[m,nsample] (SQUARED), ascending;
    equal distances by ascending point index; slots a short segment cannot fill stay (segment start, 1e10);
    1 <= nsample <= 100"""
    m, nsample = int(m), int(nsample)
    n, b = _dim0(xyz, "xyz"), _dim0(offset, "offset")
    _pn2_check((xyz, F32, "xyz", (n, 3)), (new_xyz, F32, "new_xyz", (m, 3)), (offset, I32, "offset", (b,)),
               (new_offset, I32, "new_offset", (b,)), (idx, I32, "idx", (m, nsample)), (dist2, F32, "dist2", (m, nsample)))
    if not 1 <= nsample <= _KNN_MAX:
        raise RuntimeError(f"knnquery_cuda: nsample must be in [1, {_KNN_MAX}], got {nsample}")
    call("p2pb_pointops_knnquery", b, n, m, nsample, ptr(xyz), ptr(new_xyz), ptr(offset), ptr(new_offset),
         ptr(idx), ptr(dist2), stream_ptr())


def ballquery_cuda(m, radius, nsample, xyz, new_xyz, offset, new_offset, idx):
    """PO/ballquery/ballquery_cuda.cpp. -> idx i32[m,nsample]: the first nsample points of the query's segment with
    d2 < radius^2, padded with the first; a query without one leaves its row as it is (the layer zero-fills idx first)"""
    m, nsample = int(m), int(nsample)
    n, b = _dim0(xyz, "xyz"), _dim0(offset, "offset")
    _pn2_check((xyz, F32, "xyz", (n, 3)), (new_xyz, F32, "new_xyz", (m, 3)), (offset, I32, "offset", (b,)),
               (new_offset, I32, "new_offset", (b,)), (idx, I32, "idx", (m, nsample)))
    call("p2pb_pointops_ballquery", b, n, m, radius, nsample, ptr(xyz), ptr(new_xyz), ptr(offset),
         ptr(new_offset), ptr(idx), stream_ptr())
    return 1


def furthestsampling_cuda(b, n, xyz, offset, new_offset, tmp, idx):
    """PO/sampling/sampling_cuda.cpp. `n` is the LONGEST SEGMENT (it sets the tie order: include/p2pb_hip.h), xyz f32[N,3],
    tmp f32[N] in/out (the layer fills it with 1e10) -> idx i32[new_offset[-1]], global indices"""
    b, n_max = int(b), int(n)
    n = _dim0(xyz, "xyz")
    if torch.is_tensor(idx) and idx.dim() != 1:
        raise RuntimeError(f"idx must have one dimension, got {tuple(idx.shape)}")
    _pn2_check((xyz, F32, "xyz", (n, 3)), (offset, I32, "offset", (b,)), (new_offset, I32, "new_offset", (b,)),
               (tmp, F32, "tmp", (n,)), (idx, I32, "idx", (_dim0(idx, "idx"),)))
    call("p2pb_pointops_furthestsampling", b, n, idx.shape[0], n_max, ptr(xyz), ptr(offset), ptr(new_offset),
         ptr(tmp), ptr(idx), stream_ptr())


def grouping_forward_cuda(m, nsample, c, input, idx, output):
    """PO/grouping/grouping_cuda.cpp. input f32[n,c], idx i32[m,nsample] -> output f32[m,nsample,c]"""
    m, nsample, c = int(m), int(nsample), int(c)
    _pn2_check((input, F32, "input", (_dim0(input, "input"), c)), (idx, I32, "idx", (m, nsample)),
               (output, F32, "output", (m, nsample, c)))
    call("p2pb_pointops_grouping_forward", m, nsample, c, ptr(input), ptr(idx), ptr(output), stream_ptr())


def grouping_backward_cuda(m, nsample, c, grad_output, idx, grad_input):
    """ADDS grad_output f32[m,nsample,c] at idx into grad_input f32[n,c] (fp32 atomics: refused inside
    p2p_bridge_amd.deterministic())"""
    m, nsample, c = int(m), int(nsample), int(c)
    n = _dim0(grad_input, "grad_input")
    _pn2_check((grad_output, F32, "grad_output", (m, nsample, c)), (idx, I32, "idx", (m, nsample)),
               (grad_input, F32, "grad_input", (n, c)))
    _no_scatter_in_deterministic_mode("grouping_backward_cuda")
    call("p2pb_pointops_grouping_backward", n, m, nsample, c, ptr(grad_output), ptr(idx), ptr(grad_input), stream_ptr())


def interpolation_forward_cuda(n, c, k, input, idx, weight, output):
    """PO/interpolation/interpolation_cuda.cpp. input f32[m,c], idx i32[n,k], weight f32[n,k]: ADDS the weighted rows to
    output f32[n,c] (the layer passes zeros)"""
    n, c, k = int(n), int(c), int(k)
    _pn2_check((input, F32, "input", (_dim0(input, "input"), c)), (idx, I32, "idx", (n, k)), (weight, F32, "weight", (n, k)),
               (output, F32, "output", (n, c)))
    call("p2pb_pointops_interpolation_forward", n, c, k, ptr(input), ptr(idx), ptr(weight), ptr(output), stream_ptr())


def interpolation_backward_cuda(n, c, k, grad_output, idx, weight, grad_input):
    """ADDS grad_output f32[n,c] * weight at idx into grad_input f32[m,c] (fp32 atomics: refused in deterministic mode)"""
    n, c, k = int(n), int(c), int(k)
    _pn2_check((grad_output, F32, "grad_output", (n, c)), (idx, I32, "idx", (n, k)), (weight, F32, "weight", (n, k)),
               (grad_input, F32, "grad_input", (_dim0(grad_input, "grad_input"), c)))
    _no_scatter_in_deterministic_mode("interpolation_backward_cuda")
    call("p2pb_pointops_interpolation_backward", n, c, k, ptr(grad_output), ptr(idx), ptr(weight), ptr(grad_input),
         stream_ptr())


def subtraction_forward_cuda(n, nsample, c, input1, input2, idx, output):
    """PO/subtraction/subtraction_cuda.cpp. output f32[n,nsample,c] = input1[n] - input2[idx] (written)"""
    n, nsample, c = int(n), int(nsample), int(c)
    _pn2_check((input1, F32, "input1", (n, c)), (input2, F32, "input2", (_dim0(input2, "input2"), c)),
               (idx, I32, "idx", (n, nsample)), (output, F32, "output", (n, nsample, c)))
    call("p2pb_pointops_subtraction_forward", n, nsample, c, ptr(input1), ptr(input2), ptr(idx), ptr(output),
         stream_ptr())


def subtraction_backward_cuda(n, nsample, c, idx, grad_output, grad_input1, grad_input2):
    """grad_input1[n] += the row sums of grad_output f32[n,nsample,c] (fixed order); grad_input2[idx] += -grad_output (fp32
    atomics: refused in deterministic mode). Build addition: grad_input2 = None runs the fixed-order half alone, in either mode."""
    n, nsample, c = int(n), int(nsample), int(c)
    specs = [(idx, I32, "idx", (n, nsample)), (grad_output, F32, "grad_output", (n, nsample, c)),
             (grad_input1, F32, "grad_input1", (n, c))]
    if grad_input2 is not None:
        specs.append((grad_input2, F32, "grad_input2", (_dim0(grad_input2, "grad_input2"), c)))
        _pn2_check(*specs)
        _no_scatter_in_deterministic_mode("subtraction_backward_cuda")
    else:
        _pn2_check(*specs)
    call("p2pb_pointops_subtraction_backward", n, nsample, c, ptr(idx), ptr(grad_output), ptr(grad_input1),
         ptr(grad_input2), stream_ptr())


def _aggregation_specs(n, nsample, c, w_c, input, position, weight, idx):
    if w_c < 1 or c % w_c:
        raise RuntimeError(f"aggregation: c = {c} must be a multiple of w_c = {w_c}")
    return [(input, F32, "input", (_dim0(input, "input"), c)), (position, F32, "position", (n, nsample, c)),
            (weight, F32, "weight", (n, nsample, w_c)), (idx, I32, "idx", (n, nsample))]


def aggregation_forward_cuda(n, nsample, c, w_c, input, position, weight, idx, output):
    """PO/aggregation/aggregation_cuda.cpp. ADDS sum_s (input[idx_s] + position[n,s]) * weight[n,s, ch mod w_c] to
    output f32[n,c] (the layer passes zeros); c % w_c == 0"""
    n, nsample, c, w_c = int(n), int(nsample), int(c), int(w_c)
    _pn2_check(*_aggregation_specs(n, nsample, c, w_c, input, position, weight, idx), (output, F32, "output", (n, c)))
    call("p2pb_pointops_aggregation_forward", n, nsample, c, w_c, ptr(input), ptr(position), ptr(weight),
         ptr(idx), ptr(output), stream_ptr())


def aggregation_backward_cuda(n, nsample, c, w_c, input, position, weight, idx, grad_output, grad_input, grad_position,
                              grad_weight):
    """grad_input[idx] += g w (fp32 atomics: refused in deterministic mode); grad_position = g w (WRITTEN);
    grad_weight += the per-weight-channel sums of g (input + position) (fixed order). Build addition: grad_input = None runs
    the fixed-order parts alone, in either mode."""
    n, nsample, c, w_c = int(n), int(nsample), int(c), int(w_c)
    specs = _aggregation_specs(n, nsample, c, w_c, input, position, weight, idx) + [
        (grad_output, F32, "grad_output", (n, c)), (grad_position, F32, "grad_position", (n, nsample, c)),
        (grad_weight, F32, "grad_weight", (n, nsample, w_c))]
    if grad_input is not None:
        specs.append((grad_input, F32, "grad_input", tuple(input.shape)))
        _pn2_check(*specs)
        _no_scatter_in_deterministic_mode("aggregation_backward_cuda")
    else:
        _pn2_check(*specs)
    call("p2pb_pointops_aggregation_backward", n, nsample, c, w_c, ptr(input), ptr(position), ptr(weight),
         ptr(idx), ptr(grad_output), ptr(grad_input), ptr(grad_position), ptr(grad_weight), stream_ptr())


__all__ = ["knnquery_cuda", "ballquery_cuda", "furthestsampling_cuda", "grouping_forward_cuda", "grouping_backward_cuda",
           "interpolation_forward_cuda", "interpolation_backward_cuda", "subtraction_forward_cuda", "subtraction_backward_cuda",
           "aggregation_forward_cuda", "aggregation_backward_cuda", "avg_voxelize_forward", "avg_voxelize_backward"]

# what `import pointops_cuda` resolves to after install_dropin(): the reference's 13 names and nothing else
module = types.ModuleType("pointops_cuda")
for _name in __all__:
    setattr(module, _name, globals()[_name])
