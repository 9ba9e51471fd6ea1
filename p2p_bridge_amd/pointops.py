"""The packed-batch ("offset") point operators on the gfx950 ops: the autograd Functions and callables of the reference's
third_party/openpoints/cpp/pointops/functions/pointops.py with the same names, argument order and outputs, over the 11
`*_cuda` functions of `pointops_cuda`. A batch is one packed cloud xyz f32[n,3] with cumulative segment ends offset i32[b];
features are point-major f32[n,c]; indices are int32 and global.

Two deliberate deviations from the reference, both where it fails:
  * `new_xyz=None` means `xyz` and is resolved BEFORE the contiguity check (the reference's querygroup / queryandgroup assert
    `new_xyz.is_contiguous()` first and crash on None);
  * `querygroup(..., idx=given)` groups with the given idx (the reference falls off the end of its `if idx is None` and
    returns None).
Outputs are allocated with torch.zeros / torch.full on the input's device, not the legacy torch.cuda.FloatTensor.
k-NN ranks equal distances by ascending point index (the reference: whatever its heap leaves).
"""
import torch
from torch.autograd import Function

from . import pointops_cuda as _ext

__all__ = ["FurthestSampling", "KNNQuery", "BallQuery", "Grouping", "Subtraction", "Aggregation", "Interpolation",
           "furthestsampling", "knnquery", "ballquery", "grouping", "subtraction", "aggregation", "interpolation2",
           "querygroup", "queryandgroup", "interpolation"]

F32, I32 = torch.float32, torch.int32


class FurthestSampling(Function):
    @staticmethod
    def forward(ctx, xyz, offset, new_offset):
        """xyz f32[n,3], offset i32[b], new_offset i32[b] -> idx i32[new_offset[-1]]"""
        assert xyz.is_contiguous()
        n, b = xyz.shape[0], offset.shape[0]
        ends = offset.tolist()
        n_max = max(e - s for s, e in zip([0] + ends[:-1], ends))
        idx = torch.zeros(int(new_offset[b - 1].item()), dtype=I32, device=xyz.device)
        tmp = torch.full((n,), 1e10, dtype=F32, device=xyz.device)
        _ext.furthestsampling_cuda(b, n_max, xyz, offset, new_offset, tmp, idx)
        ctx.mark_non_differentiable(idx)
        return idx


furthestsampling = FurthestSampling.apply


class KNNQuery(Function):
    @staticmethod
    def forward(ctx, nsample, xyz, new_xyz, offset, new_offset):
        """xyz f32[n,3], new_xyz f32[m,3] (None: xyz) -> idx i32[m,nsample], dist f32[m,nsample] (distances, not squares)"""
        if new_xyz is None:
            new_xyz = xyz
        assert xyz.is_contiguous() and new_xyz.is_contiguous()
        m = new_xyz.shape[0]
        idx = torch.zeros(m, nsample, dtype=I32, device=xyz.device)
        dist2 = torch.zeros(m, nsample, dtype=F32, device=xyz.device)
        _ext.knnquery_cuda(m, nsample, xyz, new_xyz, offset, new_offset, idx, dist2)
        dist = torch.sqrt(dist2)
        ctx.mark_non_differentiable(idx, dist)
        return idx, dist


knnquery = KNNQuery.apply


class BallQuery(Function):
    @staticmethod
    def forward(ctx, radius, nsample, xyz, new_xyz, offset, new_offset):
        """xyz f32[n,3], new_xyz f32[m,3] (None: xyz) -> idx i32[m,nsample]; a query without a neighbour keeps zeros"""
        if new_xyz is None:
            new_xyz = xyz
        assert xyz.is_contiguous() and new_xyz.is_contiguous()
        m = new_xyz.shape[0]
        idx = torch.zeros(m, nsample, dtype=I32, device=xyz.device)
        _ext.ballquery_cuda(m, radius, nsample, xyz, new_xyz, offset, new_offset, idx)
        ctx.mark_non_differentiable(idx)
        return idx


ballquery = BallQuery.apply


class Grouping(Function):
    @staticmethod
    def forward(ctx, input, idx):
        """input f32[n,c], idx i32[m,nsample] -> f32[m,nsample,c]"""
        assert input.is_contiguous() and idx.is_contiguous()
        m, nsample, n, c = idx.shape[0], idx.shape[1], input.shape[0], input.shape[1]
        output = torch.zeros(m, nsample, c, dtype=F32, device=input.device)
        _ext.grouping_forward_cuda(m, nsample, c, input, idx, output)
        ctx.n = n
        ctx.save_for_backward(idx)
        return output

    @staticmethod
    def backward(ctx, grad_output):
        n = ctx.n
        (idx,) = ctx.saved_tensors
        m, nsample, c = grad_output.shape
        grad_input = torch.zeros(n, c, dtype=F32, device=grad_output.device)
        _ext.grouping_backward_cuda(m, nsample, c, grad_output.contiguous(), idx, grad_input)
        return grad_input, None


grouping = Grouping.apply


def _group(xyz, new_xyz, feat, idx):
    """idx i32[m,nsample] -> (neighbour coordinates relative to their query f32[m,nsample,3], neighbour features
    f32[m,nsample,c] | None), by torch indexing"""
    rows = idx.long()
    relative = xyz[rows] - new_xyz[:, None, :]
    return relative, (feat[rows] if feat is not None else None)


def querygroup(nsample, xyz, new_xyz, feat, offset, new_offset, radius=None, query_method="knn", normalize_dp=False, idx=None):
    """k-NN ("knn" / "knnquery") or ball query (any other `query_method`, with `radius`), then `_group`
    -> (grouped_xyz f32[m,nsample,3] relative to new_xyz, grouped_feat f32[m,nsample,c] | None).
    xyz f32[n,3], new_xyz f32[m,3] (None: xyz, resolved before the contiguity check), feat f32[n,c] | None,
    idx i32[m,nsample] | None. A given idx is used as it is (the reference returns None then). `normalize_dp` divides the
    relative coordinates by `radius` for a ball query and, for query_method "knn", by each neighbour's own distance + 1e-8
    (what the reference computes: its maximum runs over the size-one last dimension). One of nsample and idx is needed
    (the reference's nsample = None branch transposes a two-dimensional tensor and raises)."""
    if new_xyz is None:
        new_xyz = xyz
    assert xyz.is_contiguous() and new_xyz.is_contiguous() and (feat is None or feat.is_contiguous())
    if idx is None:
        if nsample is None:
            raise ValueError("querygroup needs nsample or idx")
        if query_method in ("knn", "knnquery"):
            idx, _ = knnquery(nsample, xyz, new_xyz, offset, new_offset)
        else:
            idx = ballquery(radius, nsample, xyz, new_xyz, offset, new_offset)
    grouped_xyz, grouped_feat = _group(xyz, new_xyz, feat, idx)
    if normalize_dp:
        scale = torch.linalg.vector_norm(grouped_xyz, dim=-1, keepdim=True) + 1.0e-8 if query_method == "knn" else radius
        grouped_xyz = grouped_xyz / scale
    return grouped_xyz, grouped_feat


def queryandgroup(nsample, xyz, new_xyz, feat, idx, offset, new_offset, use_xyz=True):
    """-> f32[m,nsample,3+c] (relative coordinates | features), or the features alone. new_xyz = None means xyz (resolved
    before the contiguity check); idx = None runs the k-NN query."""
    if new_xyz is None:
        new_xyz = xyz
    assert xyz.is_contiguous() and new_xyz.is_contiguous() and feat.is_contiguous()
    if idx is None:
        idx, _ = knnquery(nsample, xyz, new_xyz, offset, new_offset)
    grouped_xyz, grouped_feat = _group(xyz, new_xyz, feat, idx)
    return torch.cat((grouped_xyz, grouped_feat), -1) if use_xyz else grouped_feat


class Subtraction(Function):
    @staticmethod
    def forward(ctx, input1, input2, idx):
        """input1, input2 f32[n,c], idx i32[n,nsample] -> input1[n] - input2[idx] f32[n,nsample,c]"""
        assert input1.is_contiguous() and input2.is_contiguous()
        n, c = input1.shape
        nsample = idx.shape[-1]
        output = torch.zeros(n, nsample, c, dtype=F32, device=input1.device)
        _ext.subtraction_forward_cuda(n, nsample, c, input1, input2, idx, output)
        ctx.save_for_backward(idx)
        return output

    @staticmethod
    def backward(ctx, grad_output):
        (idx,) = ctx.saved_tensors
        n, nsample, c = grad_output.shape
        grad_input1 = torch.zeros(n, c, dtype=F32, device=grad_output.device)
        grad_input2 = torch.zeros(n, c, dtype=F32, device=grad_output.device)
        _ext.subtraction_backward_cuda(n, nsample, c, idx, grad_output.contiguous(), grad_input1, grad_input2)
        return grad_input1, grad_input2, None


subtraction = Subtraction.apply


class Aggregation(Function):
    @staticmethod
    def forward(ctx, input, position, weight, idx):
        """input f32[n,c], position f32[n,nsample,c], weight f32[n,nsample,c'], idx i32[n,nsample] -> f32[n,c]"""
        assert input.is_contiguous() and position.is_contiguous() and weight.is_contiguous()
        n, nsample, c = position.shape
        w_c = weight.shape[-1]
        output = torch.zeros(n, c, dtype=F32, device=input.device)
        _ext.aggregation_forward_cuda(n, nsample, c, w_c, input, position, weight, idx, output)
        ctx.save_for_backward(input, position, weight, idx)
        return output

    @staticmethod
    def backward(ctx, grad_output):
        input, position, weight, idx = ctx.saved_tensors
        n, nsample, c = position.shape
        w_c = weight.shape[-1]
        dev = grad_output.device
        grad_input = torch.zeros(n, c, dtype=F32, device=dev)
        grad_position = torch.zeros(n, nsample, c, dtype=F32, device=dev)
        grad_weight = torch.zeros(n, nsample, w_c, dtype=F32, device=dev)
        _ext.aggregation_backward_cuda(n, nsample, c, w_c, input, position, weight, idx, grad_output.contiguous(), grad_input,
                                       grad_position, grad_weight)
        return grad_input, grad_position, grad_weight, None


aggregation = Aggregation.apply


def _inverse_distance_weights(xyz, new_xyz, offset, new_offset, k):
    idx, dist = knnquery(k, xyz, new_xyz, offset, new_offset)  # (n, k), (n, k)
    dist_recip = 1.0 / (dist + 1e-8)
    return idx, dist_recip / torch.sum(dist_recip, dim=1, keepdim=True)


def interpolation(xyz, new_xyz, feat, offset, new_offset, k=3):
    """xyz f32[m,3], new_xyz f32[n,3], feat f32[m,c] -> f32[n,c]: inverse-distance weights over the k nearest, by torch indexing"""
    assert xyz.is_contiguous() and new_xyz.is_contiguous() and feat.is_contiguous()
    idx, weight = _inverse_distance_weights(xyz, new_xyz, offset, new_offset, k)
    return (feat[idx.long()] * weight[:, :, None]).sum(1)


class Interpolation(Function):
    @staticmethod
    def forward(ctx, xyz, new_xyz, input, offset, new_offset, k=3):
        """the same on the interpolation kernels, with a gradient for `input`"""
        assert xyz.is_contiguous() and new_xyz.is_contiguous() and input.is_contiguous()
        idx, weight = _inverse_distance_weights(xyz, new_xyz, offset, new_offset, k)
        n, c, m = new_xyz.shape[0], input.shape[1], input.shape[0]
        output = torch.zeros(n, c, dtype=F32, device=input.device)
        _ext.interpolation_forward_cuda(n, c, k, input, idx, weight, output)
        ctx.m, ctx.k = m, k
        ctx.save_for_backward(idx, weight)
        return output

    @staticmethod
    def backward(ctx, grad_output):
        m, k = ctx.m, ctx.k
        idx, weight = ctx.saved_tensors
        n, c = grad_output.shape
        grad_input = torch.zeros(m, c, dtype=F32, device=grad_output.device)
        _ext.interpolation_backward_cuda(n, c, k, grad_output.contiguous(), idx, weight, grad_input)
        return None, None, grad_input, None, None, None


interpolation2 = Interpolation.apply
