"""The GroupNorm that follows a 1x1 convolution, handed to the convolution's own entry point (its fin_* arguments, csrc/common.h
GnFinish): scale / shift / channel mean must be the SAME BITS as the separate p2pb_gn_affine_params launch gives on the same
partials (the entry point puts the gn_affine launch behind the producer; round 4's in-kernel forms left the library in round 5) --
with and without AdaGN styles, ragged channel tiles, repeated launches, two streams and two host threads side by side; a shape the
norm cannot take is refused and leaves nothing behind for the calls that follow."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [  # (B, Cin, Cout, P, groups): pw_split 128- and 256-channel tiles, groups narrower and wider than a tile, the ping-pong
    (4, 64, 64, 2048, 8),     # and wide forms (finished by the launch behind them), a ragged last channel tile
    (16, 64, 128, 8192, 8),
    (8, 128, 256, 2048, 8),
    (8, 256, 512, 8192, 8),   # ping-pong at b >= 8
    (2, 256, 512, 2048, 8),   # split, 256-channel tiles? (grid decides)
    (3, 96, 192, 1024, 8),    # 192 = 128 + 64: ragged tile, cg = 24 does not nest -> launch behind
    (4, 128, 1024, 512, 8),   # cg = 128
    (2, 32, 32, 4096, 8),     # narrow: wide kernel
    (5, 64, 256, 640, 4),     # cg = 64
]


def _run(b, ci, co, p, groups, styled, want_mean, seed):
    from p2p_bridge_amd import fused

    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(b, ci, p, device="cuda", generator=g)
    conv = torch.nn.Conv1d(ci, co, 1).cuda()
    gamma = torch.randn(co, device="cuda", generator=g)
    beta = torch.randn(co, device="cuda", generator=g)
    wide = torch.randn(b, 2 * co + 40, device="cuda", generator=g)
    style = wide[:, 8:8 + 2 * co] if styled else None  # (a column slice of a wider matrix: row stride passed through)
    fin = (float(p), groups, gamma, beta, style, 1e-5, want_mean)
    with torch.no_grad():
        y, st, (sc, sh, mean) = fused.pw_conv(x, conv, fin=fin)
        y2, st2 = fused.pw_conv(x, conv)
        ref = fused.gn_affine_params(st2, float(p), groups, gamma, beta, style, 1e-5, want_mean)
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and torch.equal(st, st2)
    assert torch.equal(sc, ref[0]) and torch.equal(sh, ref[1]), (b, ci, co, p, groups, (sc - ref[0]).abs().max().item())
    assert (mean is None) == (ref[2] is None) and (mean is None or torch.equal(mean, ref[2]))
    return sc


@pytest.mark.parametrize("b,ci,co,p,groups", SHAPES)
def test_finished_by_the_producer_equals_the_separate_launch(b, ci, co, p, groups):
    for rep in range(3):
        _run(b, ci, co, p, groups, styled=rep != 1, want_mean=rep == 2, seed=rep)


def test_two_streams_side_by_side():
    from p2p_bridge_amd import fused

    torch.manual_seed(0)
    convs = [torch.nn.Conv1d(64, 128, 1).cuda() for _ in range(2)]
    xs = [torch.randn(16, 64, 8192, device="cuda") for _ in range(2)]
    gam, bet = torch.randn(128, device="cuda"), torch.randn(128, device="cuda")
    fin = (8192.0, 8, gam, bet, None, 1e-5, False)
    with torch.no_grad():
        ref = [fused.pw_conv(x, c, fin=fin)[2] for x, c in zip(xs, convs)]
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for rep in range(20):
            outs = []
            for k in range(2):
                with torch.cuda.stream(streams[k]):
                    for _ in range(4):
                        outs.append((k, fused.pw_conv(xs[k], convs[k], fin=fin)[2]))
            torch.cuda.synchronize()
            for k, (sc, sh, _) in outs:
                assert torch.equal(sc, ref[k][0]) and torch.equal(sh, ref[k][1])


def test_nothing_survives_a_refused_call():
    """the finisher travels in the call's own arguments: a call refused for its finisher's shape leaves nothing that a later call
    on the same thread, with or without a finisher, could pick up"""
    from p2p_bridge_amd import fused
    from p2p_bridge_amd._lib import P2PBError

    x = torch.randn(2, 16, 1024, device="cuda")
    conv = torch.nn.Conv1d(16, 64, 1).cuda()
    gam, bet = torch.randn(64, device="cuda"), torch.randn(64, device="cuda")
    fin = (1024.0, 8, gam, bet, None, 1e-5, True)
    with torch.no_grad():
        y0, st0 = fused.pw_conv(x, conv)
        ref = fused.gn_affine_params(st0, 1024.0, 8, gam, bet, None, 1e-5, True)
        torch.cuda.synchronize()
        bad_conv = torch.nn.Conv1d(16, 40, 1).cuda()
        one = torch.ones(40, device="cuda")
        with pytest.raises(P2PBError):
            fused.pw_conv(x, bad_conv, fin=(1024.0, 32, one, one, None, 1e-5, False))
        del one
        y1, st1 = fused.pw_conv(x, conv)
        y2, st2, aff = fused.pw_conv(x, conv, fin=fin)
    torch.cuda.synchronize()
    assert torch.equal(y1, y0) and torch.equal(st1, st0)
    assert torch.equal(y2, y0) and torch.equal(st2, st0)
    for got, want in zip(aff, ref):
        assert torch.equal(got, want)


def test_two_host_threads_side_by_side():
    """two host threads, each on its own stream with its OWN gamma / beta: every launch finishes with the norm its own call passed"""
    import threading

    from p2p_bridge_amd import fused

    b, ci, co, p, groups = 4, 64, 128, 2048, 8
    torch.manual_seed(1)
    convs = [torch.nn.Conv1d(ci, co, 1).cuda() for _ in range(2)]
    xs = [torch.randn(b, ci, p, device="cuda") for _ in range(2)]
    fins = [(float(p), groups, torch.randn(co, device="cuda"), torch.randn(co, device="cuda"), None, 1e-5, True) for _ in range(2)]
    with torch.no_grad():
        refs = [fused.pw_conv(xs[k], convs[k], fin=fins[k]) for k in range(2)]  # (also packs the weights, once, on this thread)
    torch.cuda.synchronize()
    assert not torch.equal(refs[0][2][0], refs[1][2][0])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs, errors = [[], []], []
    start = threading.Barrier(2)

    def work(k):
        try:
            with torch.no_grad(), torch.cuda.stream(streams[k]):
                start.wait(timeout=30)
                for _ in range(4):
                    outs[k].append(fused.pw_conv(xs[k], convs[k], fin=fins[k]))
                streams[k].synchronize()
        except BaseException as e:  # noqa: BLE001 (reported by the main thread)
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for k in range(2):
        assert len(outs[k]) == 4
        for y, st, aff in outs[k]:
            assert torch.equal(y, refs[k][0]) and torch.equal(st, refs[k][1])
            for got, want in zip(aff, refs[k][2]):
                assert torch.equal(got, want)


def test_a_shape_the_norm_cannot_take_is_refused():
    """cout % groups != 0 (MyGroupNorm(32, cout) with a ragged cout), cout / groups > 256 or a style row shorter than
    2 * cout used to run the finisher with a truncated group / past its LDS table; the entry point returns P2PB_EINVAL instead"""
    from p2p_bridge_amd import fused
    from p2p_bridge_amd._lib import P2PBError

    x = torch.randn(2, 16, 1024, device="cuda")
    for co, groups, style_cols in ((40, 32, None), (1040, 4, None), (64, 8, 100)):
        conv = torch.nn.Conv1d(16, co, 1).cuda()
        gam = torch.ones(co, device="cuda")
        style = None if style_cols is None else torch.randn(2, style_cols, device="cuda")
        with torch.no_grad(), pytest.raises((P2PBError, RuntimeError)):
            fused.pw_conv(x, conv, fin=(1024.0, groups, gam, gam, style, 1e-5, False))
        torch.cuda.synchronize()
