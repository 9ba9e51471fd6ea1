"""The EMD kernels (csrc/emd.hip: auction and approximate matching; csrc/setmetrics.hip: p2pb_pairwise_emd) against references
that do not share their structure: oracle/emd_check.py, itself checked on the CPU oracle by tests/test_emd_check.py.

Auction. The assignment is schedule dependent, its acceptance is not: on every case of emd_check.AUCTION_CASES (admitted on
the C oracle: one-to-one after a quarter of the rounds, so no cloud is ever skipped) and at every hand-over round of the
persistent kernel, the result is a permutation with its exact inverse, meets eps-complementary slackness against the returned
prices and costs at most n * eps more than the Hungarian optimum. A runner-up value merged wrongly across lanes, or a price
that LDS and the caller's buffer disagree on at the hand-over, breaks slackness by far more than the margin (the GetMax band
of 1e-6 plus a few roundings of fp32 values <= 3, or twice what the C oracle itself shows on the case).

Approximate matching. Kernel and C oracle are two fp32 evaluations of the same recurrences (__expf against expf, chunk-
sequential against sequential sums), so they should sit at the same order of distance from float64: the kernel is allowed 4 x
the oracle's distance on the same case (the margin tests/test_full_size_parity_gpu.py gives the oracle), with a floor of 1e-6
(1e-5 on marginals) where the oracle happens to be nearly exact. Every figure is printed before it is asserted.

Measured on an MI355X, kernel / C oracle, distance from float64 (match max abs; cost relative; worse marginal; matchcost forward
relative and backward / max |grad| on the own match):
  uniform 2x256x256    8.7e-6 / 1.7e-5   1.9e-7 / 2.1e-7   4.4e-6 / 4.0e-6   3.9e-8 / 3.3e-8   1.9e-7 / 5.5e-8
  lattice 2x256x256    7.4e-7 / 7.3e-7   3.5e-7 / 2.4e-7   6.6e-7 / 5.9e-7   1.2e-7 / 2.9e-8   2.3e-7 / 6.6e-8
  uniform 1x512x1024   1.2e-5 / 5.8e-6   2.3e-7 / 2.3e-7   7.2e-6 / 5.6e-6   3.5e-9 / 3.7e-8   5.4e-7 / 6.1e-8
  uniform 2x128x512    1.6e-6 / 2.2e-6   7.1e-8 / 7.1e-8   8.5e-7 / 7.9e-7   7.1e-9 / 2.9e-9   4.3e-7 / 6.4e-8
  uniform 1x1024x256   8.5e-7 / 8.0e-7   8.1e-7 / 6.7e-7   4.9e-5 / 4.6e-5   4.0e-8 / 3.5e-8   2.7e-7 / 8.6e-8
  uniform 2x300x200    1.4e-4 / 1.4e-4   1.1e-6 / 2.7e-6        --           1.2e-7 / 5.2e-8   1.2e-7 / 5.0e-8
  uniform 1x2048x2048  2.9e-4 / 4.1e-4   1.9e-6 / 1.1e-6   2.8e-5 / 5.8e-5   7.3e-8 / 4.1e-8   4.1e-7 / 4.0e-8
  uniform 1x1024x4096  1.3e-6 / 6.5e-7   1.9e-7 / 8.3e-8   1.4e-6 / 1.4e-6   2.0e-7 / 1.8e-8   7.1e-7 / 6.6e-8
The two matchcost kernels sum in fp32 where the oracle sums in double, hence ratios up to 11 there, all under the 1e-6 floor.
The last row is what these tests changed: with whole-tile chunks the 1024 sources were never split while the 4096 targets were
split in 4, and the kernel stood at cost 1.3e-6 (15 x the oracle) and per-target sums 4.7e-5 (34 x) -- see am_chunk_len in
csrc/emd_sweep.h. pairwise_emd: 8.4e-7 / 7.2e-7 at 256 x 256, 1.0e-6 / 2.9e-6 at 256 x 128. Auction: at every case and hand-over
round the kernels show the C oracle's own figures to all printed digits (slack - eps 1.2e-7 .. 2.3e-7, cost - optimum 0 ..
8.2e-3 against n eps = 0.128 .. 2.56); train.make_align_fn returns the Hungarian permutation.

Not guarded here: the start value of the finisher of the chunked ratio-R sums (EmdRatioR::kStart in csrc/emd_sweep.h, which
emd_finish_kernel starts from). Starting it at 1e-9f instead of 0 passes every test of
this file: 1e-9 is below half an ulp of any partial sum above 0.03, and where the partials vanish the consumption clamps to 1
and rr - 1e-9 rr == rr, so at these sizes the result does not change by a bit. That line is guarded by
tests/test_ops_parity_gpu.py::test_approxmatch_chunked_equals_single_pass, which sees the change at 1 x 4096 x 4096 (1.4e-4
against its 1.2e-5 gate) through the ill-conditioning of n == m."""
import functools

import pytest
import torch

from oracle import cpu_ops
from oracle import emd_check as C

pytestmark = pytest.mark.gpu
SLACK_MARGIN = 4e-6


@pytest.fixture(scope="module")
def met():
    from p2p_bridge_amd import metric_modules

    return metric_modules


@functools.lru_cache(maxsize=None)
def auction_reference(name):
    """clouds, Hungarian optimum and the C oracle's excess slack over eps of a case, computed once for all hand-over points"""
    case = next(c for c in C.AUCTION_CASES if c.name == name)
    x1, x2 = C.case_clouds(case)
    opt = C.hungarian(x1, x2)
    _, _, a, _, price = C.run_auction(cpu_ops.emd_assignment, x1, x2, case.eps, case.iters)
    rep = C.auction_report(x1, x2, a, price, case.eps, opt)
    assert rep.is_perm.all()
    return case, x1, x2, opt, max(0.0, rep.excess.max().item()), (rep.cost - rep.opt).max().item()


def matched_sqdist64(x1, x2, a):
    y = torch.gather(x2.double(), 1, a.long().unsqueeze(-1).expand(-1, -1, 3))
    return ((x1.double() - y) ** 2).sum(-1)


# every case at the hand-over rounds 0 (persistent from the start), 3 and 10 (the default); the never-persistent form (three
# launches per round for every round) on the 128-point cases only
AUCTION_RUNS = [(c.name, p) for c in C.AUCTION_CASES for p in (0, 3, 10)] + [(c.name, c.iters) for c in C.AUCTION_CASES if c.n == 128]


@pytest.mark.parametrize("name,persist_from", AUCTION_RUNS, ids=[f"{n}-from{p}" for n, p in AUCTION_RUNS])
def test_auction_slackness_and_optimality(met, name, persist_from, monkeypatch):
    case, x1, x2, opt, oracle_excess, oracle_gap = auction_reference(name)
    monkeypatch.setenv("P2PB_EXPERIMENT", f"auction_persist_from={persist_from}")
    rc, dist, a, inv, price = C.run_auction(met.emd_assignment, x1, x2, case.eps, case.iters, "cuda")
    rep = C.auction_report(x1, x2, a, price, case.eps, opt)
    print(f"\n{name} persist_from={persist_from}: slack - eps {[f'{s:.3e}' for s in rep.excess.tolist()]} (oracle "
          f"{oracle_excess:.3e}), cost - optimum {[f'{g:.3e}' for g in (rep.cost - rep.opt).tolist()]} (oracle at most "
          f"{oracle_gap:.3e}, n eps = {case.n * case.eps:g})")
    assert rc == 1
    assert rep.is_perm.all(), "a cloud was left without a one-to-one assignment"
    assert torch.equal(torch.gather(inv.long(), 1, a.long()), torch.arange(case.n).expand_as(a))
    assert (dist.double() - matched_sqdist64(x1, x2, a)).abs().max().item() <= 1e-6
    assert (price >= 0).all()
    assert (rep.excess <= max(SLACK_MARGIN, 2 * oracle_excess)).all(), rep.slack
    assert (rep.cost >= rep.opt - 1e-9).all() and (rep.cost <= rep.opt + case.n * (case.eps + SLACK_MARGIN)).all()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU")
def test_auction_persistent_tail_on_second_device(met, monkeypatch):
    """One process, the auction on device 0 and then on device 1 at 1 x 4096: the persistent tail needs 18 * 4096 = 73,728 B
    of LDS, above the 64 KB a kernel gets without opting in, and the opt-in holds per device. A launcher that opts in once per
    process has the second launch refused (rc 0). The cloud is a shuffled copy under noise 0.012: the C oracle is one-to-one
    after round 11 and before round 14, so the tail (from round 10) still moves objects and 30 rounds leave a margin."""
    monkeypatch.delenv("P2PB_EXPERIMENT", raising=False)
    n = 4096
    g = torch.Generator().manual_seed(0)
    x2 = torch.rand(1, n, 3, generator=g)
    x1 = (x2[:, torch.randperm(n, generator=g)] + 0.012 * torch.randn(1, n, 3, generator=g)).contiguous()
    for dev in ("cuda:0", "cuda:1"):
        with torch.cuda.device(dev):
            rc, _, a, inv, _ = C.run_auction(met.emd_assignment, x1, x2, 0.01, 30, dev)
        assert rc == 1, dev
        assert torch.equal(a.long().sort(1).values, torch.arange(n).expand_as(a)), dev
        assert torch.equal(torch.gather(inv.long(), 1, a.long()), torch.arange(n).expand_as(a)), dev


def test_align_fn_returns_the_hungarian_permutation(monkeypatch):
    """train.make_align_fn (eps 0.01, 100 rounds, [B,3,N] layout) on the shuffled noisy copies: the C oracle reaches the
    optimum itself there (tests/test_emd_check.py), so the aligned clean patch is the Hungarian permutation of the clean
    points; were the kernel's own schedule to end elsewhere, its cost is held to the auction's bound instead"""
    from p2p_bridge_amd import train as T

    monkeypatch.delenv("P2PB_EXPERIMENT", raising=False)
    case, x1, x2, (opt_cost, opt_a), _, _ = auction_reference(C.ALIGN_CASE)
    assert (case.eps, case.iters) == (0.01, 100)
    noisy, clean = x1.transpose(1, 2).contiguous(), x2.transpose(1, 2).contiguous()
    aligned = T.make_align_fn()(noisy.cuda(), clean.cuda()).cpu()
    want = torch.gather(clean, 2, opt_a.unsqueeze(1).expand(-1, 3, -1))
    assert aligned.shape == clean.shape
    # every aligned column is a clean point, every clean point is used once
    same = (aligned.unsqueeze(3) == clean.unsqueeze(2)).all(1)  # [b, aligned i, clean k]
    assert (same.sum(2) == 1).all() and (same.sum(1) == 1).all()
    gap = (aligned.double() - noisy.double()).norm(dim=1).sum(1) - opt_cost
    print(f"\nalign_fn: cost - optimum {[f'{g:.3e}' for g in gap.tolist()]}")
    if not torch.equal(aligned, want):
        assert (gap >= -1e-9).all() and (gap <= case.n * (case.eps + SLACK_MARGIN)).all()


@functools.lru_cache(maxsize=None)
def approx_reference(case):
    x1, x2 = C.approx_clouds(case)
    ref = C.approxmatch64(x1, x2)
    gc = C.grad_cost_of(case)
    return x1, x2, gc, ref, C.approx_errors(cpu_ops.emd_cuda, x1, x2, gc, ref)[0]


@pytest.mark.parametrize("case", C.APPROX_CASES, ids=lambda c: f"{c.kind}-{c.b}x{c.n}x{c.m}")
def test_approxmatch_and_matchcost_against_float64(met, case):
    from p2p_bridge_amd._lib import lib

    b, n, m = case.b, case.n, case.m
    chunks = {(1, 2048, 2048): 2, (1, 1024, 4096): 4}.get((b, n, m), 1)
    temp = int(lib().p2pb_approxmatch_temp_floats(b, n, m))
    assert temp == 2 * (n + m) * b + (chunks * b * max(n, m) if chunks > 1 else 0)  # (the chunked launches: PART + finisher)
    x1, x2, gc, ref, eo = approx_reference(case)
    eh, match = C.approx_errors(met.emd_cuda, x1, x2, gc, ref, "cuda")
    print(f"\n{case}\n  oracle - fp64 {eo}\n  hip    - fp64 {eh}\n  ratios " +
          ", ".join(f"{k} {getattr(eh, k) / getattr(eo, k):.2f}" for k in ("match", "cost", "cost_kernel", "grad") if getattr(eo, k) > 0))
    assert eh.match <= max(4 * eo.match, 1e-6)
    assert eh.cost <= max(4 * eo.cost, 1e-6)
    assert eh.min_entry >= 0
    if C.divisible(n, m):
        assert eh.marg_l <= max(4 * eo.marg_l, 1e-5) and eh.marg_r <= max(4 * eo.marg_r, 1e-5)
    assert eh.cost_kernel <= max(4 * eo.cost_kernel, 1e-6)
    assert eh.grad <= max(4 * eo.grad, 1e-6)


@pytest.mark.parametrize("n,m", [(256, 256), (256, 128)])
def test_pairwise_emd_against_float64(n, m):
    """p2pb_pairwise_emd never stores a match matrix: S x R costs / n against approxmatch64's, the C oracle's distance taken pair
    by pair (it has no pairwise entry point) and every pair held to 4 x ITS oracle distance, floor 1e-6 (measured: the worst pair
    stands at 3.3 x of max(oracle, floor / 4) at 256 x 256, 1.0 x at 256 x 128); a roomy workspace and one for 5 of the 12 pairs
    at a time"""
    from p2p_bridge_amd import evaluation_metrics_fast as E

    S, R = 3, 4
    g = torch.Generator().manual_seed(11)
    A, B = torch.rand(S, n, 3, generator=g), torch.rand(R, m, 3, generator=g)
    x1, x2 = A.repeat_interleave(R, 0).contiguous(), B.repeat(S, 1, 1).contiguous()  # pair p = (p // R, p % R)
    want = (C.approxmatch64(x1, x2)[1] / n).view(S, R)
    m0 = cpu_ops.approxmatch_forward(x1, x2)
    eo = (((cpu_ops.matchcost_forward(x1, x2, m0) / float(n)).double().view(S, R) - want).abs() / want)
    roomy = E.pairwise_emd(A.cuda(), B.cuda())
    small = E.pairwise_emd(A.cuda(), B.cuda(), ws_bytes=5 * (3 * n + 2 * m) * 4)
    assert roomy.shape == (S, R) and roomy.dtype == torch.float32
    for what, got in (("roomy", roomy), ("5 pairs at a time", small)):
        eh = ((got.cpu().double() - want).abs() / want)
        print(f"\npairwise_emd {n} x {m}, {what}: hip - fp64 {eh.max().item():.3e}, oracle - fp64 {eo.max().item():.3e} relative "
              f"(ratio {eh.max().item() / eo.max().item():.2f}; worst single pair {(eh / eo.clamp(min=2.5e-7)).max().item():.2f})")
        assert (eh <= (4 * eo).clamp(min=1e-6)).all(), (eh, eo)  # the 4 x rule pair by pair
    assert torch.equal(roomy, small)
