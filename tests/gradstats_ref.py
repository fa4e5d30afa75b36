"""Torch-fp64 restatement of rvt_grad_stats (csrc/gradstats.hpp) for tests/test_gradmonitor.py: the statistics of one tensor from its
fp32 gradient and parameter values, computed on the CPU in double.

BOUND of every sum comparison (`sum_bound`): a sum of n non-negative double terms, added in any order, is within
(n - 1) * 2^-53 * sum|term| of the exact sum to first order (Higham, Accuracy and Stability of Numerical Algorithms, 4.2); the terms
themselves are exact here (|g| and p are fp32 values, g^2 and p^2 have 48 significant bits).  The kernel's sum and torch's sum
each carry at most that error, so they differ by at most n * 2^-52 * sum|term|: the bound the issue states, derived, not measured."""
import math

import torch


def tensor_stats(g: torch.Tensor, p: torch.Tensor) -> dict:
    """g, p: fp32 tensors of one parameter (any device).  Non-finite = inf or NaN by IEEE classification on the CPU."""
    g32, p32 = g.detach().cpu().reshape(-1), p.detach().cpu().reshape(-1)
    assert g32.dtype == torch.float32 and p32.dtype == torch.float32
    gf, pf = torch.isfinite(g32), torch.isfinite(p32)
    gd, pd = g32[gf].double(), p32[pf].double()
    return dict(numel=g32.numel(), nonfinite=int((~gf).sum()), n_finite=int(gf.sum()), n_param_finite=int(pf.sum()),
                abs_sum=float(gd.abs().sum()), sq_sum=float((gd * gd).sum()), param_sq_sum=float((pd * pd).sum()),
                abs_max=float(g32[gf].abs().max()) if bool(gf.any()) else 0.0)


def sum_bound(n_terms: int, total: float) -> float:
    """n * 2^-52 * sum|term| for a sum of non-negative terms whose (reference) value is `total`."""
    return n_terms * 2.0 ** -52 * abs(total)


def check_tensor(what: str, got: dict, want: dict) -> None:
    """got: one entry of GradMonitor.read()[...]['params']; want: tensor_stats().  Exact: counts and the maximum; bounded: the sums."""
    assert got['numel'] == want['numel'], (what, got['numel'], want['numel'])
    assert got['nonfinite'] == want['nonfinite'], (what, got['nonfinite'], want['nonfinite'])
    assert got['grad_abs_max'] == want['abs_max'], (what, got['grad_abs_max'], want['abs_max'])
    for key, ref, n in (('grad_abs_sum', 'abs_sum', want['n_finite']), ('grad_sq_sum', 'sq_sum', want['n_finite']),
                        ('param_sq_sum', 'param_sq_sum', want['n_param_finite'])):
        err, bound = abs(got[key] - want[ref]), sum_bound(n, want[ref])
        assert math.isfinite(got[key]) and err <= bound, (what, key, got[key], want[ref], err, bound)
    assert got['grad_abs_mean'] == got['grad_abs_sum'] / want['numel']
    assert got['grad_norm'] == math.sqrt(got['grad_sq_sum']) and got['param_norm'] == math.sqrt(got['param_sq_sum'])


def check_head(what: str, got: dict, wants: list) -> None:
    """got: one record of GradMonitor.read(); wants: tensor_stats() of every tensor of the optimizer's table, in table order."""
    assert got['nonfinite'] == sum(w['nonfinite'] for w in wants), what
    assert got['grad_abs_max'] == max(w['abs_max'] for w in wants), what
    total = math.fsum(w['sq_sum'] for w in wants)
    n = sum(w['n_finite'] for w in wants)
    assert abs(got['grad_sq_sum'] - total) <= sum_bound(n, total), (what, got['grad_sq_sum'], total)
    assert got['global_grad_norm'] == math.sqrt(got['grad_sq_sum'])
