"""The classic PointNet++ surface of the drop-in module without a GPU: the nine names exist and none has a CPU path."""
import pytest
import torch

F32, I32 = torch.float32, torch.int32
B, C, N, M, U = 1, 2, 16, 4, 3


def z(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype)


# name -> arguments in the reference's pybind order, on the CPU
CALLS = {
    "ball_query_wrapper": (B, N, M, 0.5, U, z(B, M, 3), z(B, N, 3), z(B, M, U, dtype=I32)),
    "group_points_wrapper": (B, C, N, M, U, z(B, C, N), z(B, M, U, dtype=I32), z(B, C, M, U)),
    "group_points_grad_wrapper": (B, C, N, M, U, z(B, C, M, U), z(B, M, U, dtype=I32), z(B, C, N)),
    "gather_points_wrapper": (B, C, N, M, z(B, C, N), z(B, M, dtype=I32), z(B, C, M)),
    "gather_points_grad_wrapper": (B, C, N, M, z(B, C, M), z(B, M, dtype=I32), z(B, C, N)),
    "furthest_point_sampling_wrapper": (B, N, M, z(B, N, 3), z(B, N), z(B, M, dtype=I32)),
    "three_nn_wrapper": (B, N, M, z(B, N, 3), z(B, M, 3), z(B, N, 3), z(B, N, 3, dtype=I32)),
    "three_interpolate_wrapper": (B, C, M, N, z(B, C, M), z(B, N, 3, dtype=I32), z(B, N, 3), z(B, C, N)),
    "three_interpolate_grad_wrapper": (B, C, N, M, z(B, C, N), z(B, N, 3, dtype=I32), z(B, N, 3), z(B, C, M)),
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_wrapper_exists_and_refuses_cpu_tensors(name):
    from p2p_bridge_amd import pointnet2_batch_cuda as ext

    fn = getattr(ext, name)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        fn(*CALLS[name])
    for t in CALLS[name]:
        if torch.is_tensor(t):
            assert not t.any()  # nothing was computed on the host


def test_operator_api_names_and_no_cpu_path():
    from p2p_bridge_amd import pointnet2_ops as ops

    for name in ("FurthestPointSampling", "GatherOperation", "GroupingOperation", "BallQuery", "ThreeNN", "ThreeInterpolate"):
        assert issubclass(getattr(ops, name), torch.autograd.Function), name
    for name in ("furthest_point_sample", "gather_operation", "grouping_operation", "ball_query", "three_nn", "three_interpolate"):
        assert callable(getattr(ops, name)), name
    with pytest.raises(RuntimeError):
        ops.furthest_point_sample(z(B, N, 3), M)
    with pytest.raises(RuntimeError):
        ops.three_interpolate(z(B, C, M).requires_grad_(), z(B, N, 3, dtype=I32), z(B, N, 3))
