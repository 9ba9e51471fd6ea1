"""The classic PointNet++ operator API on the gfx950 ops: the six autograd Functions of the reference's layers
(third_party/openpoints/models/layers/subsample.py:73, group.py:82,145,181, upsampling.py:9,40) with the same names,
argument order, outputs and ctx attributes, and their lower-case callables, over the nine `*_wrapper` functions of
`pointnet2_batch_cuda`. Clouds are point-major f32[B,N,3], features channel-major f32[B,C,N], indices int32.
The modules built on them (`QueryAndGroup`, `GroupAll`, ...) are plain torch over these callables and are not mirrored here.
fp32 only; inside autocast the feature operators cast their inputs to fp32, as the reference's do.
"""
import torch
from torch.autograd import Function

from . import pointnet2_batch_cuda as _ext

__all__ = ["FurthestPointSampling", "GatherOperation", "GroupingOperation", "BallQuery", "ThreeNN", "ThreeInterpolate",
           "furthest_point_sample", "gather_operation", "grouping_operation", "ball_query", "three_nn", "three_interpolate"]

_fp32_inputs = torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)


class FurthestPointSampling(Function):
    @staticmethod
    def forward(ctx, xyz, npoint):
        """xyz f32[B,N,3] -> i32[B,npoint]: iterative furthest point sampling from point 0"""
        B, N, _ = xyz.size()
        output = torch.empty(B, npoint, dtype=torch.int32, device=xyz.device)
        temp = torch.empty(B, N, dtype=torch.float32, device=xyz.device).fill_(1e10)
        _ext.furthest_point_sampling_wrapper(B, N, npoint, xyz, temp, output)
        ctx.mark_non_differentiable(output)
        return output

    @staticmethod
    def backward(ctx, a=None):
        return None, None


furthest_point_sample = FurthestPointSampling.apply


class GatherOperation(Function):
    @staticmethod
    def forward(ctx, features, idx):
        """features f32[B,C,N], idx i32[B,npoint] -> f32[B,C,npoint]"""
        B, npoint = idx.size()
        _, C, N = features.size()
        output = torch.empty(B, C, npoint, dtype=torch.float32, device=features.device)
        _ext.gather_points_wrapper(B, C, N, npoint, features, idx, output)
        ctx.for_backwards = (idx, C, N)
        return output

    @staticmethod
    def backward(ctx, grad_out):
        idx, C, N = ctx.for_backwards
        B, npoint = idx.size()
        grad_features = torch.zeros(B, C, N, dtype=torch.float32, device=grad_out.device)
        _ext.gather_points_grad_wrapper(B, C, N, npoint, grad_out.detach().contiguous(), idx, grad_features)
        return grad_features, None


gather_operation = GatherOperation.apply


class GroupingOperation(Function):
    @staticmethod
    @_fp32_inputs
    def forward(ctx, features, idx):
        """features f32[B,C,N], idx i32[B,npoint,nsample] -> f32[B,C,npoint,nsample]"""
        B, npoint, nsample = idx.size()
        _, C, N = features.size()
        output = torch.empty(B, C, npoint, nsample, dtype=torch.float32, device=features.device)
        _ext.group_points_wrapper(B, C, N, npoint, nsample, features, idx, output)
        ctx.for_backwards = (idx, N)
        return output

    @staticmethod
    def backward(ctx, grad_out):
        idx, N = ctx.for_backwards
        B, C, npoint, nsample = grad_out.size()
        grad_features = torch.zeros(B, C, N, dtype=torch.float32, device=grad_out.device)
        _ext.group_points_grad_wrapper(B, C, N, npoint, nsample, grad_out.detach().contiguous(), idx, grad_features)
        return grad_features, None


grouping_operation = GroupingOperation.apply


class BallQuery(Function):
    @staticmethod
    def forward(ctx, radius, nsample, xyz, new_xyz):
        """xyz f32[B,N,3], new_xyz f32[B,npoint,3] -> i32[B,npoint,nsample]; a ball without a point keeps the zero fill"""
        B, N, _ = xyz.size()
        npoint = new_xyz.size(1)
        idx = torch.zeros(B, npoint, nsample, dtype=torch.int32, device=xyz.device)
        _ext.ball_query_wrapper(B, N, npoint, radius, nsample, new_xyz, xyz, idx)
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, a=None):
        return None, None, None, None


ball_query = BallQuery.apply


class ThreeNN(Function):
    @staticmethod
    def forward(ctx, unknown, known):
        """unknown f32[B,N,3], known f32[B,m,3] -> (dist f32[B,N,3]: the l2 distances, ascending; idx i32[B,N,3])"""
        B, N, _ = unknown.size()
        m = known.size(1)
        dist2 = torch.empty(B, N, 3, dtype=torch.float32, device=unknown.device)
        idx = torch.empty(B, N, 3, dtype=torch.int32, device=unknown.device)
        _ext.three_nn_wrapper(B, N, m, unknown, known, dist2, idx)
        dist = torch.sqrt(dist2)
        ctx.mark_non_differentiable(dist, idx)
        return dist, idx

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None


three_nn = ThreeNN.apply


class ThreeInterpolate(Function):
    @staticmethod
    @_fp32_inputs
    def forward(ctx, features, idx, weight):
        """features f32[B,c,m], idx i32[B,n,3], weight f32[B,n,3] -> f32[B,c,n]"""
        B, c, m = features.size()
        n = idx.size(1)
        ctx.three_interpolate_for_backward = (idx, weight, m)
        output = torch.empty(B, c, n, dtype=torch.float32, device=features.device)
        _ext.three_interpolate_wrapper(B, c, m, n, features, idx, weight, output)
        return output

    @staticmethod
    def backward(ctx, grad_out):
        idx, weight, m = ctx.three_interpolate_for_backward
        B, c, n = grad_out.size()
        grad_features = torch.zeros(B, c, m, dtype=torch.float32, device=grad_out.device)
        _ext.three_interpolate_grad_wrapper(B, c, n, m, grad_out.detach().contiguous(), idx, weight, grad_features)
        return grad_features, None, None


three_interpolate = ThreeInterpolate.apply
