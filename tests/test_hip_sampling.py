"""The hip backend of the sampling ops on the MI355X against the CPU goldens (oracle/sampling.py).

Tolerances (none comes from the code under test):

* indices and gathered values are exact: the tie rule makes the top K unique;
* the cut: the golden's fp32 running sum decides ``cum > top_p``; another summation order may decide differently only where
  the sum sits on the threshold.  A row is *undecidable* when the fp64 running sum comes within ``delta`` of ``top_p`` at any
  position, ``delta = 8 x`` the largest |fp32 - fp64| running-sum deviation of the golden on that case (8: a tree-ordered
  scan against a sequential one).  There the cut may differ by one position and the probabilities are compared against the
  golden re-evaluated with that cut; everywhere else the kept set is exact.  At most 5 % of a case may be undecidable;
* probabilities: relative error against an fp64 evaluation at most 8 x the golden's own fp32 error against it on the same
  case; for 16-bit outputs one unit in the last place of the output dtype.

Every test prints the figures it asserts on.
"""
import pytest
import torch

import mojo_opset_amd as mo
import oracle.sampling as G
from conftest import bit_equal, clone_tree, load_golden, to_device
from sampling_judge import Judged, _cdf_targets, _check_draw, _ulps, final64  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NEG_INF = -float("inf")
CASES = load_golden("sampling")
FILTER = [c for c in CASES if c["op"] == "MojoTopPFilter"]
SAMPLERS = [c for c in CASES if c["op"] in ("MojoTopKSampling", "MojoTopPSampling")]
PENALTIES = [c for c in CASES if c["op"] == "MojoApplyPenaltiesTempurate"]
REJECT = [c for c in CASES if c["op"] in ("MojoRejectSampling", "MojoJoinProbRejectSampling")]


def _S():
    from mojo_opset_amd.backends.hip.operators import sampling as S

    return S


def _hip(name, **kwargs):
    return getattr(mo, name).get_backend_impl("hip", strict=True)(**kwargs)


def _ids(cases):
    return [pytest.param(c, id=f"{c['op'][4:]}-{i}") for i, c in enumerate(cases)]


def _run_filter(logits, top_p, keep, k, filter_value=NEG_INF, slices=0):
    probs, indices = _S().top_p_filter(logits.to(DEV), top_p, keep, k, filter_value, slices)
    torch.cuda.synchronize()
    return probs, indices


@pytest.mark.parametrize("case", _ids(FILTER))
def test_filter_on_the_fixture_cases(case):
    logits, top_p, keep, k = case["args"]
    fv = case["ctor"]["kwargs"]["filter_value"]
    probs, indices = _hip("MojoTopPFilter", filter_value=fv)(logits.to(DEV), top_p, keep, k)
    kk = min(k, logits.shape[-1])
    assert probs.shape == indices.shape == logits.shape[:-1] + (kk,)
    assert torch.equal(indices.cpu(), case["out"][1])
    assert torch.equal(torch.gather(logits, -1, indices.cpu()), torch.gather(logits, -1, case["out"][1]))
    Judged(logits, top_p, keep, k, fv).check(probs, indices, logits.dtype, f"fixture {tuple(logits.shape)} {logits.dtype}")


LARGE = [  # rows, vocab, k, top_p, scale, dtype, seed
    (20, 151936, 1000, 0.75, 1.0, torch.float32, 0),
    (60, 155136, 100, 0.7, 1.0, torch.float32, 1),
    (120, 151936, 1000, 0.7, 1.0, torch.float32, 0),
    (33, 151936, 10, 0.75, 1.0, torch.float32, 1),
    (64, 128256, 1000, 0.75, 4.0, torch.float32, 0),
    (32, 151936, 1000, 0.75, 1.0, torch.bfloat16, 1),
    (16, 128256, 1024, 0.9, 1.0, torch.float16, 0),
    (7, 50001, 300, 0.8, 2.0, torch.float32, 1),           # an odd vocabulary: rows are not 16-byte aligned
]


def _logits(rows, vocab, scale, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, vocab, generator=g) * scale).to(dtype)


@pytest.mark.parametrize("rows,vocab,k,top_p,scale,dtype,seed", LARGE)
def test_filter_on_vocabulary_sized_rows(rows, vocab, k, top_p, scale, dtype, seed):
    logits = _logits(rows, vocab, scale, dtype, seed)
    if dtype != torch.float32:
        top = torch.sort(logits.float(), dim=-1, descending=True).values[:, :k + 1]
        print(f"tied neighbours in the top {k + 1}: {int((top[:, 1:] == top[:, :-1]).sum())}")
    probs, indices = _run_filter(logits, top_p, 1, k)
    judged = Judged(logits, top_p, 1, k, NEG_INF)
    assert torch.equal(torch.gather(logits.float(), -1, indices.cpu()), judged.values)
    judged.check(probs, indices, dtype, f"({rows}, {vocab}) K {k} {dtype}")
    removed = torch.arange(k).expand(rows, k) >= (judged.kept + judged.undecidable.long()).unsqueeze(-1)
    assert not probs.cpu()[removed].any()                                       # exactly 0 past the cut


def test_filter_with_minus_infinity_logits_and_min_tokens():
    logits = _logits(9, 32768, 1.0, torch.float32, 0)
    logits[:, 5000:] = NEG_INF                                                  # a masked vocabulary
    logits[3, 100:] = NEG_INF                                                   # fewer finite logits than K
    probs, indices = _run_filter(logits, 0.6, 4, 256, NEG_INF)
    Judged(logits, 0.6, 4, 256, NEG_INF).check(probs, indices, torch.float32, "-inf logits")
    probs, indices = _run_filter(logits[:3], 0.6, 2, 256, -4.0)
    Judged(logits[:3], 0.6, 2, 256, -4.0).check(probs, indices, torch.float32, "finite filter value")


@pytest.mark.parametrize("rows,vocab,k,dtype", [(20, 151936, 1000, torch.float32), (5, 40000, 333, torch.bfloat16),
                                                (3, 2000, 2000 // 2, torch.float16)])
def test_every_slice_count_gives_the_same_bits(rows, vocab, k, dtype):
    from mojo_opset_amd.backends.hip import lib as L

    logits = _logits(rows, vocab, 1.0, dtype, 0)
    base = _run_filter(logits, 0.75, 1, k)
    forms = {L.last_launch()}
    for slices in (1, 2, 3, 5, 8, 4096):
        assert bit_equal(_run_filter(logits, 0.75, 1, k, slices=slices), base), f"slices={slices}"
        forms.add(L.last_launch())
    print(sorted(forms))
    assert all(f.startswith("sampling:filter:top_p:slices") for f in forms) and len(forms) >= 2
    u = torch.rand(rows, device=DEV)
    picks = [_S().sample_with_uniforms(logits.to(DEV), u, k, top_p=0.75, slices=s) for s in (0, 1, 2, 3, 5, 8, 4096)]
    assert all(bit_equal(p, picks[0]) for p in picks[1:])
    assert L.last_launch().startswith("sampling:sample:top_p:slices")


@pytest.mark.parametrize("rows,vocab,k,top_p,dtype,seed", [(20, 151936, 1000, 0.75, torch.float32, 0),
                                                           (60, 155136, 100, 0.7, torch.float32, 1),
                                                           (24, 128256, 50, None, torch.bfloat16, 0)])
def test_selection_with_a_given_uniform(rows, vocab, k, top_p, dtype, seed):
    S = _S()
    logits = _logits(rows, vocab, 1.0, dtype, seed)
    dev_logits = logits.to(DEV)
    if top_p is None:                                                           # the top-k form: nothing removed
        values, indices = G.topk_sorted(logits.float(), k)
        judged = Judged(logits, 2.0, 1, k, NEG_INF)
        assert bool((judged.kept == k).all()) and torch.equal(judged.indices, indices)
    else:
        judged = Judged(logits, top_p, 1, k, NEG_INF)
    usable = ~judged.undecidable
    assert float(usable.float().mean()) >= 0.95
    skipped = total = 0
    g = torch.Generator().manual_seed(seed)
    for name, target, u, width in _cdf_targets(judged, rows, g):
        probs, tokens = S.sample_with_uniforms(dev_logits, u.to(DEV), k, top_p=top_p)
        assert probs.shape == tokens.shape == (rows, 1) and probs.dtype == torch.float32 and tokens.dtype == torch.int64
        judge = usable & (width >= judged.delta)
        skipped += int((~judge).sum())
        total += rows
        want_tok = judged.indices.gather(-1, target[:, None])[:, 0]
        want_p = judged.ref64.gather(-1, target[:, None])[:, 0]
        assert torch.equal(tokens.cpu()[:, 0][judge], want_tok[judge]), name
        err = ((probs.cpu()[:, 0].double() - want_p).abs() / want_p)[judge].max()
        print(f"{name}: relative error of the returned probability {float(err):.3e} (bound {judged.tol:.3e})")
        assert float(err) <= judged.tol
    print(f"intervals narrower than delta or on undecidable rows: {skipped} of {total}")
    assert skipped <= 0.05 * total
    zero = S.sample_with_uniforms(dev_logits, torch.zeros(rows, device=DEV), k, top_p=top_p)
    assert torch.equal(zero[1].cpu()[:, 0], judged.indices[:, 0])               # u = 0: the first token
    top = torch.full((rows,), float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))), device=DEV)
    probs, tokens = S.sample_with_uniforms(dev_logits, top, k, top_p=top_p)
    assert bool((probs > 0).all())                                              # never a removed token
    pos = (judged.indices == tokens.cpu()).float().argmax(-1)
    assert bool((pos < judged.kept + judged.undecidable.long()).all())


def test_an_even_grid_of_uniforms_reproduces_the_distribution():
    n, vocab, k = 4096, 8192, 64
    row = _logits(1, vocab, 2.0, torch.float32, 1)
    judged = Judged(row, 0.9, 1, k, NEG_INF)
    assert not bool(judged.undecidable.any())
    u = (torch.arange(n, dtype=torch.float32) / n).to(DEV)
    probs, tokens = _S().sample_with_uniforms(row.to(DEV).expand(n, vocab), u, k, top_p=0.9)
    tokens = tokens.cpu()[:, 0]
    counts = (tokens[:, None] == judged.indices[0][None, :]).sum(0).double() / n
    assert float(counts.sum()) == 1.0
    worst = float((counts - judged.ref64[0]).abs().max())
    print(f"largest |count / {n} - probability| = {worst:.3e} (bound {2 / n:.3e})")
    assert worst <= 2 / n
    assert bool((tokens[1:] != tokens[:-1]).sum() == int((counts > 0).sum()) - 1)   # monotone in u


def _judged_sampler(name, kwargs, logits):
    vocab = logits.shape[-1]
    if name == "MojoTopKSampling":                                              # nothing removed: a top_p no running sum reaches
        k = max(min(kwargs.get("top_k", 50), vocab), kwargs.get("min_tokens_to_keep", 1))
        return Judged(logits, 2.0, 1, k, NEG_INF)
    return Judged(logits, kwargs.get("top_p", 0.75), kwargs.get("min_tokens_to_keep", 1), kwargs.get("rand_top_k", 1000),
                  kwargs.get("filter_value", NEG_INF))


@pytest.mark.parametrize("case", _ids(SAMPLERS))
def test_public_samplers_on_the_fixture_cases(case):
    logits = case["args"][0]
    judged = _judged_sampler(case["op"], case["ctor"]["kwargs"], logits)
    assert torch.equal(judged.indices, case["out"][1].reshape(judged.indices.shape))
    assert float(judged.undecidable.float().mean()) <= 0.05
    op = _hip(case["op"], **case["ctor"]["kwargs"])
    for _ in range(8):
        probs, tokens = op(logits.to(DEV))
        assert probs.shape == tokens.shape == logits.shape[:-1] + (1,)
        assert probs.dtype == torch.float32 and tokens.dtype == torch.int64
        _check_draw(judged, probs, tokens, case["op"])


@pytest.mark.parametrize("name,kwargs", [("MojoTopKSampling", {"top_k": 20}), ("MojoTopPSampling", {"top_p": 0.7, "rand_top_k": 1000})])
def test_public_samplers_on_vocabulary_sized_rows(name, kwargs):
    rows, vocab = 64, 151936
    logits = _logits(rows, vocab, 1.0, torch.float32, 0)
    op = _hip(name, **kwargs)
    judged = _judged_sampler(name, kwargs, logits)
    assert float(judged.undecidable.float().mean()) <= 0.05
    dev_logits = logits.to(DEV)
    torch.manual_seed(11)
    first = op(dev_logits)
    second = op(dev_logits)                                                     # no reseed: other uniforms
    torch.manual_seed(11)
    again = op(dev_logits)
    assert bit_equal(first, again)
    assert int((first[1] != second[1]).sum()) >= 1
    for probs, tokens in (first, second):
        assert probs.shape == tokens.shape == (rows, 1) and probs.dtype == torch.float32 and tokens.dtype == torch.int64
        _check_draw(judged, probs, tokens, name)


def test_zero_rows_and_one_dimensional_logits():
    S = _S()
    probs, indices = S.top_p_filter(torch.empty(0, 1000, device=DEV), 0.75, 1, 50)
    assert probs.shape == indices.shape == (0, 50) and indices.dtype == torch.int64
    probs, tokens = _hip("MojoTopPSampling")(torch.empty(0, 1000, device=DEV))
    assert probs.shape == tokens.shape == (0, 1)
    probs, tokens = _hip("MojoTopKSampling", top_k=5)(torch.randn(999, device=DEV))
    assert probs.shape == tokens.shape == (1,)


def _one_ulp(out, want):
    if want.dtype == torch.float32:
        return bit_equal(out, want)
    return out.dtype == want.dtype and int(_ulps(out.cpu(), want).max()) <= 1


@pytest.mark.parametrize("case", _ids(PENALTIES))
def test_penalties_on_the_fixture_cases(case):
    args = list(to_device(clone_tree(case["args"]), DEV))
    args[1:2] = [[None if f is None else (f if i % 2 else f.cpu()) for i, f in enumerate(args[1])]]   # some rows arrive on the CPU
    out = _hip("MojoApplyPenaltiesTempurate")(*args)
    assert _one_ulp(out, case["out"])
    if case["args"][0].dtype == torch.float32:
        assert out is args[0]
    else:
        assert torch.equal(args[0].cpu(), case["args"][0])


@pytest.mark.parametrize("dtype,fdtype", [(torch.float32, torch.int32), (torch.float32, torch.float32), (torch.bfloat16, torch.int64),
                                          (torch.float16, torch.int32)])
def test_penalties_on_vocabulary_sized_rows(dtype, fdtype):
    rows, vocab = 20, 151936
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(rows, vocab, generator=g) * 3).to(dtype)
    freqs = [None if i % 5 == 4 else (torch.randint(1, 6, (vocab,), generator=g) * (torch.rand(vocab, generator=g) < 0.05)).to(fdtype)
             for i in range(rows)]
    presence = [0.0 if i % 3 == 0 else 0.1 * i for i in range(rows)]
    frequency = [0.0 if i % 4 == 1 else 0.05 * i for i in range(rows)]
    repetition = [1.0 if i % 6 == 2 else 0.8 + 0.05 * i for i in range(rows)]
    temps = [None if i % 7 == 3 else 0.5 + 0.1 * i for i in range(rows)]
    want = G.TorchApplyPenaltiesTempurate()(logits.clone(), freqs, presence, frequency, repetition, temps)
    dev_logits = logits.to(DEV)
    out = _hip("MojoApplyPenaltiesTempurate")(dev_logits, [None if f is None else f.to(DEV) for f in freqs], presence, frequency,
                                              repetition, temps)
    assert _one_ulp(out, want)
    if dtype == torch.float32:
        assert out is dev_logits and not torch.equal(dev_logits.cpu(), logits)   # modified in place
    else:
        assert torch.equal(dev_logits.cpu(), logits)
        print(f"{dtype}: elements that differ from the golden {int((out.cpu() != want).sum())}")


def _reject_both_ways(name, target, tokens, draft, seed):
    joint = name == "MojoJoinProbRejectSampling"
    batch, steps = tokens.shape
    torch.manual_seed(seed)
    u = torch.rand(batch, steps if joint else 1, device=DEV)                    # what the operator draws after the same seed
    got = _hip(name)(target.to(DEV), tokens.to(DEV), draft.to(DEV), random_seed=seed)
    want = getattr(G, "Torch" + name[4:])()(target, tokens, draft, uniforms=u.cpu())
    assert bit_equal(got, want), (got[1].tolist(), want[1].tolist())
    return want[1]


@pytest.mark.parametrize("case", _ids(REJECT))
def test_reject_samplers_on_the_fixture_cases(case):
    lens = _reject_both_ways(case["op"], *case["args"], seed=case["kwargs"]["random_seed"])
    assert lens.dtype == (torch.int32 if "Join" in case["op"] else torch.int64)


@pytest.mark.parametrize("name", ["MojoRejectSampling", "MojoJoinProbRejectSampling"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_reject_samplers_on_a_vocabulary_sized_batch(name, dtype):
    batch, steps, vocab = 15, 3, 155136
    g = torch.Generator().manual_seed(9)
    target = torch.softmax(torch.randn(batch, steps + 1, vocab, generator=g) * 3, dim=-1)
    tokens = torch.randint(0, vocab, (batch, steps), generator=g)
    picked = torch.gather(target[:, :steps], -1, tokens.unsqueeze(-1)).squeeze(-1)
    draft = picked / (torch.rand(batch, steps, generator=g) * 2 + 1e-3)         # ratios spread over (0, 2)
    seen = set()
    for seed in (0, 1, 2, 3):
        seen.update(_reject_both_ways(name, target.to(dtype), tokens, draft.to(dtype), seed).tolist())
    print(name, dtype, "accepted lengths seen:", sorted(seen))
    assert len(seen) >= 3


def test_filter_and_selection_replay_from_a_graph():
    S = _S()
    rows, vocab, k = 16, 151936, 1000
    batches = [_logits(rows, vocab, 1.0, torch.float32, s) for s in (0, 1, 2)]
    us = [torch.rand(rows, generator=torch.Generator().manual_seed(s)) for s in (0, 1, 2)]
    static_logits, static_u = batches[0].to(DEV), us[0].to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                              # warm-up outside the capture
        S.top_p_filter(static_logits, 0.75, 1, k)
        S.sample_with_uniforms(static_logits, static_u, k, top_p=0.75)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        filtered = S.top_p_filter(static_logits, 0.75, 1, k)
        picked = S.sample_with_uniforms(static_logits, static_u, k, top_p=0.75)
    for logits, u in zip(batches[1:], us[1:]):
        static_logits.copy_(logits)
        static_u.copy_(u)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in (*filtered, *picked)]
        eager = (*S.top_p_filter(logits.to(DEV), 0.75, 1, k), *S.sample_with_uniforms(logits.to(DEV), u.to(DEV), k, top_p=0.75))
        assert bit_equal(replayed, list(eager))
