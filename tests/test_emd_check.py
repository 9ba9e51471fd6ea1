"""oracle/emd_check.py (exact optima for the auction, a float64 restatement of approximate matching) checked on the CPU oracle,
so that tests/test_emd_exact_gpu.py stands on references that are known to be right and on cases that are known to be usable.

Auction: every case of emd_check.AUCTION_CASES must already be one-to-one on the C oracle after a QUARTER of its rounds (the
admission condition: the GPU test never has to skip or exempt a cloud); with all rounds the oracle's result meets
eps-complementary slackness against its own prices and lands within n * eps of the Hungarian optimum.

Approximate matching: the C oracle (fp32, expf) sits as close to approxmatch64 as its precision allows. Each case is held to
TWICE the distance measured on it when the cases were fixed (emd_check.ORACLE_MEASURED: match matrix, relative cost, the worse
marginal, case by case; the two matchcost kernels, whose error is only the rounding of fp32 terms summed in double, by their
largest figure over the cases). The GPU file allows the kernels 4 x the oracle's distance, so these gates are what keeps that
yardstick from drifting: neither a broken restatement nor a worse oracle can hide behind a wide gate."""
import pytest
import torch

from oracle import cpu_ops
from oracle import emd_check as C

SLACK_MARGIN = 4e-6  # the 1e-6 band of GetMax plus a few roundings of fp32 values of magnitude <= 3 (ulp 2.4e-7)


@pytest.mark.parametrize("case", C.AUCTION_CASES, ids=lambda c: c.name)
def test_auction_case_is_admitted_and_the_oracle_meets_the_exact_criteria(case):
    x1, x2 = C.case_clouds(case)
    opt = C.hungarian(x1, x2)
    rc, _, a, _, price = C.run_auction(cpu_ops.emd_assignment, x1, x2, case.eps, case.iters // 4)
    assert rc == 1
    assert C.auction_report(x1, x2, a, price, case.eps, opt).is_perm.all(), "not one-to-one after a quarter of the rounds"
    rc, dist, a, inv, price = C.run_auction(cpu_ops.emd_assignment, x1, x2, case.eps, case.iters)
    rep = C.auction_report(x1, x2, a, price, case.eps, opt)
    print(f"\n{case.name}: slack - eps {[f'{s:.3e}' for s in rep.excess.tolist()]}, cost - optimum "
          f"{[f'{g:.3e}' for g in (rep.cost - rep.opt).tolist()]} (n eps = {case.n * case.eps:g})")
    assert rc == 1 and rep.is_perm.all()
    assert torch.equal(torch.gather(inv.long(), 1, a.long()), torch.arange(case.n).expand_as(a))
    assert (price >= 0).all()
    assert (rep.excess <= SLACK_MARGIN).all(), rep.slack
    assert (rep.cost >= rep.opt - 1e-9).all() and (rep.cost <= rep.opt + case.n * (case.eps + SLACK_MARGIN)).all()
    if case.name == C.ALIGN_CASE:  # the wrapper-level check of the GPU file expects the Hungarian permutation itself
        assert torch.equal(a.long(), rep.opt_assignment)


def test_auction_cases_cover_what_the_gpu_test_needs():
    kinds = {(kind, c.n, c.eps, c.iters) for c in C.AUCTION_CASES for kind, _, _ in c.clouds}
    assert any(k == "uniform" for k, *_ in kinds)
    assert any(k == "noisy" and (eps, it) in ((1e-2, 100), (5e-3, 50)) for k, _, eps, it in kinds)
    assert any(n >= 1024 for _, n, _, _ in kinds)
    mixed = [c for c in C.AUCTION_CASES if len(c.clouds) == 3]
    assert mixed and {k for k, _, _ in mixed[0].clouds} == {"noisy", "uniform", "identical"}
    assert any(c.n == 128 for c in C.AUCTION_CASES)  # (the never-persistent form runs on these)
    assert len({c.name for c in C.AUCTION_CASES}) == len(C.AUCTION_CASES) and C.ALIGN_CASE in {c.name for c in C.AUCTION_CASES}


def test_auction_report_notices_a_worse_assignment():
    """the report is a measurement, not a verdict: a swapped pair breaks slackness and raises the cost, a repeated target is no
    permutation, and the Hungarian assignment under the optimal dual prices has slack 0"""
    case = next(c for c in C.AUCTION_CASES if c.name == C.ALIGN_CASE)
    x1, x2 = C.case_clouds(case)
    _, _, a, _, price = C.run_auction(cpu_ops.emd_assignment, x1, x2, case.eps, case.iters)
    good = C.auction_report(x1, x2, a, price, case.eps)
    swapped = a.clone()
    swapped[:, [0, 1]] = a[:, [1, 0]]
    bad = C.auction_report(x1, x2, swapped, price, case.eps, (good.opt, good.opt_assignment))
    assert bad.is_perm.all() and (bad.cost > good.cost + 10 * case.eps).all() and (bad.slack > 10 * case.eps).all()
    twice = a.clone()
    twice[:, 0] = a[:, 1]
    assert not C.auction_report(x1, x2, twice, price, case.eps, (good.opt, good.opt_assignment)).is_perm.any()
    # brute force on 6 points: the optimum is the best of all 720 permutations
    import itertools

    y1, y2 = C.auction_clouds("uniform", 1, 6, 5)
    D = torch.cdist(y1.double(), y2.double())[0]
    best = min(sum(D[j, p[j]].item() for j in range(6)) for p in itertools.permutations(range(6)))
    assert abs(C.hungarian(y1, y2)[0].item() - best) < 1e-12


def _gates(case):
    """twice the recorded distance of the C oracle from float64 on this case"""
    got = C.ORACLE_MEASURED[case]
    return dict(match=2 * got["match"], cost=2 * got["cost"], marg=2 * got["marg"] if got["marg"] is not None else None,
                cost_kernel=2 * C.ORACLE_MEASURED_COST_KERNEL, grad=2 * C.ORACLE_MEASURED_GRAD)


@pytest.mark.parametrize("case", C.APPROX_CASES, ids=lambda c: f"{c.kind}-{c.b}x{c.n}x{c.m}")
def test_approxmatch64_against_the_c_oracle(case):
    x1, x2 = C.approx_clouds(case)
    ref = C.approxmatch64(x1, x2)
    err, _ = C.approx_errors(cpu_ops.emd_cuda, x1, x2, C.grad_cost_of(case), ref)
    print(f"\n{case}: oracle against fp64 {err}")
    g = _gates(case)
    assert err.match <= g["match"] and err.cost <= g["cost"]
    assert err.cost_kernel <= g["cost_kernel"] and err.grad <= g["grad"]
    assert err.min_entry >= 0 and ref[0].min().item() >= 0
    if C.divisible(case.n, case.m):  # a transport plan: exact marginals, in float64 up to the 1e-9 regularisers
        assert max(err.marg_l, err.marg_r) <= g["marg"]
        assert max(C.marginal_errors(ref[0], case.n, case.m)) <= 1e-6
        assert ref[2].max().item() <= 1e-6 and ref[3].max().item() <= 1e-6  # nothing left to place
    multiL, multiR = C.multipliers(case.n, case.m)
    assert multiL * case.n == multiR * case.m or not C.divisible(case.n, case.m)


def test_approx_cases_cover_what_the_gpu_test_needs():
    sizes = [(c.b, c.n, c.m) for c in C.APPROX_CASES if c.kind == "uniform"]
    assert sizes == [(2, 256, 256), (1, 512, 1024), (2, 128, 512), (1, 1024, 256), (2, 300, 200), (1, 2048, 2048), (1, 1024, 4096)]
    assert [(c.b, c.n, c.m) for c in C.APPROX_CASES if c.kind == "lattice"] == [(2, 256, 256)]
    x1, x2 = C.approx_clouds(next(c for c in C.APPROX_CASES if c.kind == "lattice"))
    assert ((x1 * 4) == (x1 * 4).round()).all() and (torch.cdist(x1[0], x2[0]) == 0).any()  # duplicates across the clouds


def test_matchcost_grads64_is_the_closed_form():
    """d/dx1_k = 2 g sum_l match[l,k] (x1_k - x2_l), d/dx2_l = 2 g sum_k match[l,k] (x2_l - x1_k)"""
    case = C.ApproxCase("uniform", 2, 40, 24, 3)
    x1, x2 = C.approx_clouds(case)
    match = torch.rand(2, 24, 40, generator=torch.Generator().manual_seed(4)).double()
    gc = C.grad_cost_of(case)
    g1, g2 = C.matchcost_grads64(x1, x2, match, gc)
    d = x1.double().unsqueeze(2) - x2.double().unsqueeze(1)  # [b,n,m,3]
    w = match.transpose(1, 2).unsqueeze(-1) * gc.double().view(-1, 1, 1, 1)
    assert torch.allclose(g1, (2 * w * d).sum(2), rtol=1e-12, atol=1e-14)
    assert torch.allclose(g2, (-2 * w * d).sum(1), rtol=1e-12, atol=1e-14)
