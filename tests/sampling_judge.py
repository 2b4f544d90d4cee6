"""How a filter or sampler result is judged against the CPU goldens (oracle/sampling.py); shared by
tests/test_hip_sampling.py, tests/test_hip_sampling_pin.py and, on the host, tests/test_sampling_pin_golden.py.

Tolerances (none comes from the code under test):

* indices and gathered values are exact: the tie rule makes the top K unique;
* the cut: the golden's fp32 running sum decides ``cum > top_p``; another summation order may decide differently only where
  the sum sits on the threshold.  A row is *undecidable* when the fp64 running sum comes within ``delta`` of ``top_p`` at any
  position, ``delta = 8 x`` the largest |fp32 - fp64| running-sum deviation of the golden on that case (8: a tree-ordered
  scan against a sequential one).  There the cut may differ by one position and the probabilities are compared against the
  golden re-evaluated with that cut; everywhere else the kept set is exact.  At most ``cap`` of a case may be undecidable
  (5 % on random rows; 0 on the constructed rows of tests/sampling_pin.py, whose ``top_p`` is chosen off the running sum);
* probabilities: relative error against an fp64 evaluation at most 8 x the golden's own fp32 error against it on the same
  case; for 16-bit outputs one unit in the last place of the output dtype.
"""
import torch

import oracle.sampling as G


def _ulps(a, b):
    """Distance in units of the last place between two tensors of one 16-bit dtype (same sign or zero)."""
    return (a.view(torch.int16).int() - b.view(torch.int16).int()).abs()


def final64(values, kept, filter_value):
    """``final_probs_dist`` in fp64 with the first ``kept[row]`` positions kept."""
    k = values.shape[-1]
    removed = torch.arange(k).expand(values.shape) >= kept.unsqueeze(-1)
    return torch.softmax(values.double().masked_fill(removed, filter_value), dim=-1)


class Judged:
    """The golden's view of one filter call on 2-D fp32 values: cut, tolerance, undecidable rows (module docstring)."""

    def __init__(self, logits, top_p, keep, k, filter_value):
        x = logits.reshape(-1, logits.shape[-1])
        self.k = min(k, x.shape[-1])
        self.filter_value = filter_value
        self.probs32, self.indices, self.values = G.top_p_filter(x, top_p, keep, k, filter_value)
        cum32 = self.values.softmax(-1).cumsum(-1)
        cum64 = torch.softmax(self.values.double(), -1).cumsum(-1)
        self.delta = 8 * float((cum32.double() - cum64).abs().max())
        threshold = float(torch.tensor(top_p, dtype=torch.float32))               # what the fp32 comparison sees
        self.nearest = float((cum64 - threshold).abs().min())
        self.undecidable = ((cum64 - threshold).abs() < self.delta).any(-1)
        self.kept = (~G.removed_mask(cum32, top_p, keep)).sum(-1)
        self.ref64 = final64(self.values, self.kept, filter_value)
        big = self.ref64 > 1e-30
        self.golden_err = float(((self.probs32.double() - self.ref64).abs() / self.ref64.clamp(min=1e-300))[big].max())
        self.tol = 8 * self.golden_err

    def check(self, probs, indices, dtype, what, cap=0.05):
        rows = self.values.shape[0]
        probs, indices = probs.reshape(rows, self.k).cpu(), indices.reshape(rows, self.k).cpu()
        assert indices.dtype == torch.int64 and probs.dtype == dtype
        assert torch.equal(indices, self.indices), f"{what}: indices differ from the golden's"
        frac = float(self.undecidable.float().mean())
        print(f"{what}: delta {self.delta:.3e} nearest approach {self.nearest:.3e} undecidable rows {int(self.undecidable.sum())} "
              f"of {rows}; golden fp32 error {self.golden_err:.3e} -> tolerance {self.tol:.3e}")
        assert frac <= cap
        worst = torch.full((rows,), float("inf"), dtype=torch.float64)
        for shift in (0, -1, 1):
            kept = (self.kept + shift).clamp(1, self.k)
            ref = final64(self.values, kept, self.filter_value)
            allowed = self.undecidable if shift else torch.ones(rows, dtype=torch.bool)
            if dtype == torch.float32:
                big = ref > 1e-30
                err = ((probs.double() - ref).abs() / ref.clamp(min=1e-300)).masked_fill(~big, 0.0).amax(-1)
                err = torch.where(((probs != 0) & (ref == 0)).any(-1), torch.full_like(err, float("inf")), err)
                ok_zero = ((probs == 0) | (ref > 0)).all(-1)                   # removed positions exactly 0 under -inf
                err = torch.where(ok_zero, err, torch.full_like(err, float("inf")))
            else:
                err = _ulps(probs, ref.to(dtype)).amax(-1).double()
            worst = torch.where(allowed, torch.minimum(worst, err), worst)
        bound = self.tol if dtype == torch.float32 else 1.0
        print(f"{what}: worst {'relative error' if dtype == torch.float32 else 'ulp distance'} {float(worst.max()):.3e} (bound {bound:.3e})")
        assert float(worst.max()) <= bound


def _cdf_targets(judged, rows, g):
    """For the first, the last kept and a random kept position of every row: the fp32 midpoint of its interval of the fp64 CDF."""
    cdf = judged.ref64.cumsum(-1)
    cdf = cdf / cdf[:, -1:]
    lower = torch.cat([torch.zeros(rows, 1, dtype=torch.float64), cdf[:, :-1]], dim=-1)
    last = judged.kept - 1
    rand = (torch.rand(rows, generator=g) * judged.kept).long().clamp(max=judged.k - 1)
    for name, target in (("first", torch.zeros(rows, dtype=torch.long)), ("last kept", last), ("random kept", rand)):
        lo, hi = lower.gather(-1, target[:, None])[:, 0], cdf.gather(-1, target[:, None])[:, 0]
        yield name, target, ((lo + hi) / 2).float(), hi - lo


def _check_draw(judged, probs, tokens, what):
    rows = judged.values.shape[0]
    probs, tokens = probs.reshape(rows, 1).cpu(), tokens.reshape(rows, 1).cpu()
    where = judged.indices == tokens
    assert bool((where.sum(-1) == 1).all())                                     # a token of the candidate set ...
    want = judged.ref64[where]
    ok = ~judged.undecidable
    assert bool((want[ok] > 0).all()) and bool((probs > 0).all())               # ... that the golden keeps ...
    err = float(((probs[:, 0].double() - want).abs() / want)[ok].max())
    print(f"{what}: relative error of the returned probability {err:.3e} (bound {judged.tol:.3e})")
    assert err <= judged.tol                                                    # ... with its probability
