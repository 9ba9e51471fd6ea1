"""Schedule-independent references for the two EMD flavours of csrc/emd.hip (and p2pb_pairwise_emd of csrc/setmetrics.hip),
computed plainly with torch / numpy / scipy in float64 on the CPU (never the product, never the C oracle).

Auction (emd_assignment). Whatever order the bids land in, once every bidder holds an object the result must satisfy
eps-complementary slackness against the returned prices: bidder j's net value 3 - |x1_j - x2_a(j)| - price[a(j)] is within eps
of its best net value over all objects. The transport cost sum_j |x1_j - x2_a(j)| (distances, not squared) is then within
n * eps of the optimum of the assignment problem, which scipy.optimize.linear_sum_assignment gives exactly. auction_report
measures both; AUCTION_CASES is the one list of clouds / eps / rounds that tests/test_emd_check.py admits on the C oracle
(every cloud one-to-one after a quarter of the rounds) and tests/test_emd_exact_gpu.py then holds the kernels to.

Approximate matching (PyTorchEMD). Ten annealing levels of dense matrix arithmetic: approxmatch64 restates the kernels in
float64, matchcost_grads64 differentiates the cost with the match held constant. When one cloud size divides the other the
result is a transport plan: every source row of `match` sums to multiL, every target row to multiR."""
from collections import namedtuple

import numpy as np
import torch

F64 = torch.float64

# ------------------------------------------------------------------------------------------------------------ auction

AuctionCase = namedtuple("AuctionCase", "name clouds n eps iters")  # clouds: ((kind, b, seed), ...) concatenated along the batch
AuctionReport = namedtuple("AuctionReport", "is_perm slack excess cost opt opt_assignment")  # one entry per cloud

AUCTION_CASES = (
    AuctionCase("uniform128-s0", (("uniform", 2, 0),), 128, 1e-3, 10000),
    AuctionCase("uniform128-s1", (("uniform", 2, 1),), 128, 1e-3, 10000),
    AuctionCase("uniform128-s2", (("uniform", 2, 2),), 128, 1e-3, 10000),
    AuctionCase("uniform256-s0", (("uniform", 2, 0),), 256, 1e-3, 10000),
    AuctionCase("noisy1024-eval", (("noisy", 2, 0),), 1024, 1e-3, 10000),
    AuctionCase("noisy256-train", (("noisy", 2, 0),), 256, 1e-2, 100),  # train.make_align_fn's setting
    AuctionCase("noisy512-loss", (("noisy", 2, 0),), 512, 5e-3, 50),  # the EMD loss's setting
    # three clouds that finish in very different rounds: the persistent kernel's workgroups leave one by one
    AuctionCase("mixed128", (("noisy", 1, 0), ("uniform", 1, 0), ("identical", 1, 0)), 128, 1e-3, 10000),
)
ALIGN_CASE = "noisy256-train"  # the case the wrapper-level check (train.make_align_fn) runs on


def auction_clouds(kind, b, n, seed):
    """-> (x1, x2) f32 [b,n,3]: x1 are the bidders, x2 the objects"""
    g = torch.Generator().manual_seed(seed)
    if kind == "uniform":
        x1, x2 = torch.rand(b, n, 3, generator=g), torch.rand(b, n, 3, generator=g)
    elif kind == "noisy":  # a shuffled copy of x2 under noise: the training pair (short optimal distances, few rounds)
        x2 = torch.rand(b, n, 3, generator=g)
        x1 = x2[:, torch.randperm(n, generator=g)] + 0.02 * torch.randn(b, n, 3, generator=g)
    elif kind == "identical":  # all-zero optimal distances: sqrtf(0), value ties resolved by lowest index
        x2 = torch.rand(b, n, 3, generator=g)
        x1 = x2.clone()
    else:
        raise ValueError(kind)
    return x1.contiguous(), x2.contiguous()


def case_clouds(case):
    parts = [auction_clouds(kind, b, case.n, seed) for kind, b, seed in case.clouds]
    return torch.cat([p[0] for p in parts]).contiguous(), torch.cat([p[1] for p in parts]).contiguous()


def run_auction(mod, x1, x2, eps, iters, device="cpu"):
    """(the one harness among the references, shared by both test files so that oracle and kernels get identical buffers)
    emd_assignment.forward of `mod` (the C oracle's or the product's drop-in) on fresh state buffers laid out as
    metrics/emd_assignment/emd_module.py does -> (rc, dist, assignment, assignment_inv, price), on the CPU"""
    b, n, _ = x1.shape
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=device)
    dist, assignment, inv, price = z(b, n), z(b, n, dt=torch.int32) - 1, z(b, n, dt=torch.int32) - 1, z(b, n)
    rc = mod.forward(x1.to(device), x2.to(device), dist, assignment, price, inv, z(b, n, dt=torch.int32), z(b, n), z(b, n),
                     z(b * n, dt=torch.int32), z(512, dt=torch.int32), z(512, dt=torch.int32), z(512, dt=torch.int32),
                     z(b * n, dt=torch.int32), eps, iters)
    return rc, dist.cpu(), assignment.cpu(), inv.cpu(), price.cpu()


def hungarian(x1, x2):
    """the exact optimum of the assignment problem on plain distances -> (cost f64[b], assignment i64[b,n])"""
    from scipy.optimize import linear_sum_assignment

    D = torch.cdist(x1.to(F64), x2.to(F64)).numpy()
    cost, cols = [], []
    for d in D:
        r, c = linear_sum_assignment(d)
        assert np.array_equal(r, np.arange(d.shape[0]))
        cost.append(d[r, c].sum())
        cols.append(c)
    return torch.tensor(cost, dtype=F64), torch.from_numpy(np.stack(cols)).long()


def auction_report(x1, x2, assignment, price, eps, opt=None):
    """per cloud, in float64: is the assignment a permutation; the largest shortfall of a bidder's net value against its best
    net value under the returned prices, and its excess over eps (eps-complementary slackness asks for none); the transport
    cost; the Hungarian optimum. `opt` takes a hungarian() result computed before."""
    b, n, _ = x1.shape
    a = assignment.long().cpu()
    D = torch.cdist(x1.cpu().to(F64), x2.cpu().to(F64))
    is_perm = torch.tensor([bool(a[i].min() >= 0 and a[i].max() < n and a[i].unique().numel() == n) for i in range(b)])
    value = 3.0 - D - price.cpu().to(F64).unsqueeze(1)  # [b, bidder, object]
    held = torch.gather(value, 2, a.clamp(0, n - 1).unsqueeze(-1)).squeeze(-1)
    slack = (value.max(2).values - held).max(1).values
    cost = torch.gather(D, 2, a.clamp(0, n - 1).unsqueeze(-1)).squeeze(-1).sum(1)
    opt_cost, opt_a = hungarian(x1, x2) if opt is None else opt
    return AuctionReport(is_perm, slack, slack - float(eps), cost, opt_cost, opt_a)


# ------------------------------------------------------------------------------------------------- approximate matching

ApproxCase = namedtuple("ApproxCase", "kind b n m seed")

APPROX_CASES = (
    ApproxCase("uniform", 2, 256, 256, 1),
    ApproxCase("lattice", 2, 256, 256, 1),  # exact duplicates, exp(0)
    ApproxCase("uniform", 1, 512, 1024, 1),
    ApproxCase("uniform", 2, 128, 512, 1),
    ApproxCase("uniform", 1, 1024, 256, 1),
    ApproxCase("uniform", 2, 300, 200, 1),  # neither size divides the other: no marginal check
    ApproxCase("uniform", 1, 2048, 2048, 1),  # the chunked launches, 2 chunks
    ApproxCase("uniform", 1, 1024, 4096, 1),  # the chunked launches, 4 chunks
)
# The C oracle's distance from float64 on each case (approx_errors' fields match, cost, worse marginal, cost_kernel, grad), as
# measured when the cases were fixed. tests/test_emd_check.py holds the oracle to twice these, case by case, so the yardstick
# that tests/test_emd_exact_gpu.py multiplies by 4 cannot drift. cost_kernel and grad are fp32 results of double sums: what is
# left is the rounding of the terms and of the result (half an ulp is 6e-8), so one figure each serves every case.
ORACLE_MEASURED = {
    APPROX_CASES[0]: dict(match=1.74e-5, cost=2.12e-7, marg=4.01e-6),
    APPROX_CASES[1]: dict(match=7.35e-7, cost=2.41e-7, marg=5.87e-7),
    APPROX_CASES[2]: dict(match=5.77e-6, cost=2.30e-7, marg=5.56e-6),
    APPROX_CASES[3]: dict(match=2.21e-6, cost=7.13e-8, marg=7.94e-7),
    APPROX_CASES[4]: dict(match=8.04e-7, cost=6.66e-7, marg=4.59e-5),
    APPROX_CASES[5]: dict(match=1.44e-4, cost=2.74e-6, marg=None),
    APPROX_CASES[6]: dict(match=4.15e-4, cost=1.06e-6, marg=5.84e-5),
    APPROX_CASES[7]: dict(match=6.46e-7, cost=8.32e-8, marg=1.42e-6),
}
ORACLE_MEASURED_COST_KERNEL = 5.2e-8  # the largest of the eight cases (2.9e-9 .. 5.2e-8)
ORACLE_MEASURED_GRAD = 8.6e-8  # the largest of the eight cases (4.0e-8 .. 8.6e-8)


def approx_clouds(case):
    """-> (x1 f32 [b,n,3], x2 f32 [b,m,3]); `lattice` draws from the 5^3 points of a quarter-unit grid"""
    g = torch.Generator().manual_seed(case.seed)
    if case.kind == "uniform":
        return torch.rand(case.b, case.n, 3, generator=g), torch.rand(case.b, case.m, 3, generator=g)
    if case.kind == "lattice":
        return (torch.randint(0, 5, (case.b, case.n, 3), generator=g).float() / 4,
                torch.randint(0, 5, (case.b, case.m, 3), generator=g).float() / 4)
    raise ValueError(case.kind)


def multipliers(n, m):
    """(multiL, multiR): the mass of one source / one target point"""
    return (1.0, float(n // m)) if n >= m else (float(m // n), 1.0)


def divisible(n, m):
    return max(n, m) % min(n, m) == 0


def sqdist64(x1, x2):
    """squared distances f64 [b,n,m] of the f32 inputs"""
    d = x1.to(F64).unsqueeze(2) - x2.to(F64).unsqueeze(1)
    return (d * d).sum(-1)


def approxmatch64(x1, x2):
    """csrc/emd.hip's am_* kernels in float64 -> (match [b,m,n], cost [b], remainL [b,n], remainR [b,m])"""
    b, n, _ = x1.shape
    m = x2.shape[1]
    D = sqdist64(x1, x2)
    multiL, multiR = multipliers(n, m)
    remainL = torch.full((b, n), multiL, dtype=F64)
    remainR = torch.full((b, m), multiR, dtype=F64)
    match = torch.zeros(b, m, n, dtype=F64)
    for j in range(7, -3, -1):
        level = -(4.0 ** j) if j != -2 else 0.0
        K = torch.exp(level * D)
        suml = 1e-9 + torch.einsum("bnm,bm->bn", K, remainR)
        ratioL = remainL / suml
        sumr = torch.einsum("bnm,bn->bm", K, ratioL) * remainR
        ratioR = torch.clamp(remainR / (sumr + 1e-9), max=1.0) * remainR
        remainR = torch.clamp(remainR - sumr, min=0.0)
        W = K * ratioL.unsqueeze(2) * ratioR.unsqueeze(1)
        match += W.transpose(1, 2)
        remainL = torch.clamp(remainL - W.sum(2), min=0.0)
    cost = (D * match.transpose(1, 2)).sum((1, 2))
    return match, cost, remainL, remainR


def matchcost64(x1, x2, match):
    """sum_kl d_kl match[l,k] in float64 -> [b]"""
    return (sqdist64(x1, x2) * match.to(F64).transpose(1, 2)).sum((1, 2))


def matchcost_grads64(x1, x2, match, grad_cost):
    """float64 autograd of sum_b grad_cost_b * sum D * match with `match` held constant -> (g1 [b,n,3], g2 [b,m,3])"""
    a = x1.to(F64).clone().requires_grad_(True)
    c = x2.to(F64).clone().requires_grad_(True)
    d = a.unsqueeze(2) - c.unsqueeze(1)
    total = (grad_cost.to(F64) * ((d * d).sum(-1) * match.detach().to(F64).transpose(1, 2)).sum((1, 2))).sum()
    g1, g2 = torch.autograd.grad(total, (a, c))
    return g1, g2


ApproxErrors = namedtuple("ApproxErrors", "match cost marg_l marg_r min_entry cost_kernel grad")


def grad_cost_of(case):
    """the upstream gradient of the per-cloud costs every comparison of a case uses: f32 [b] in [0.5, 1.5)"""
    return torch.rand(case.b, generator=torch.Generator().manual_seed(100 + case.seed)) + 0.5


def approx_errors(ops, x1, x2, grad_cost, ref, device="cpu"):
    """the distances of one fp32 implementation (`ops`: approxmatch_forward / matchcost_forward / matchcost_backward, the C
    oracle's or the product's) from float64, `ref` = approxmatch64(x1, x2):
      match        max |match - match64|
      cost         max relative |matchcost_forward(own match) - cost64|
      marg_l/r     marginal_errors of the own match
      min_entry    the smallest entry of the own match
      cost_kernel  max relative |matchcost_forward(own match) - float64 sum D * own match|      (that kernel alone)
      grad         max |matchcost_backward(own match) - matchcost_grads64(own match)| / max |grad64|, the worse of g1, g2
    -> (ApproxErrors, own match on the CPU)"""
    (b, n, _), m = x1.shape, x2.shape[1]
    m64, c64 = ref[0], ref[1]
    a, c = x1.to(device), x2.to(device)
    match_dev = ops.approxmatch_forward(a, c)
    cost = ops.matchcost_forward(a, c, match_dev).cpu().to(F64)
    grads = [g.cpu().to(F64) for g in ops.matchcost_backward(grad_cost.to(device), a, c, match_dev)]
    match = match_dev.cpu()
    own = matchcost64(x1, x2, match)
    g64 = matchcost_grads64(x1, x2, match, grad_cost)
    marg_l, marg_r = marginal_errors(match, n, m)
    err = ApproxErrors(match=(match.to(F64) - m64).abs().max().item(), cost=((cost - c64).abs() / c64).max().item(),
                       marg_l=marg_l, marg_r=marg_r, min_entry=match.min().item(),
                       cost_kernel=((cost - own).abs() / own).max().item(),
                       grad=max(((g - r).abs().max() / r.abs().max()).item() for g, r in zip(grads, g64)))
    return err, match


def marginal_errors(match, n, m):
    """(max |sum over targets - multiL|, max |sum over sources - multiR|) of match [b,m,n], summed in float64"""
    multiL, multiR = multipliers(n, m)
    mt = match.to(F64)
    return (mt.sum(1) - multiL).abs().max().item(), (mt.sum(2) - multiR).abs().max().item()
