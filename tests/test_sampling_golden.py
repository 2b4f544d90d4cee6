"""The sampling ops without a GPU: the goldens against the recorded reference outputs, the tie rule, what the fixture must
contain, dispatch and registration, `SAMPLING_OPS`, the plugin's registration, the host-side refusals of the hip classes and
the workspace query.

The recorded outputs (oracle/make_sampling_golden.py) are one file under the 1 MiB bound of a committed file."""
import os
import sys
import types

import pytest
import torch

import mojo_opset_amd as mo
import oracle.sampling as G
from conftest import GOLDEN, bit_equal, clone_tree, load_golden
from mojo_opset_amd.core import MojoOperator
from mojo_opset_amd.core.platform import get_platform

OPS = ("MojoTopKSampling", "MojoTopPSampling", "MojoTopPFilter", "MojoRejectSampling", "MojoJoinProbRejectSampling",
       "MojoApplyPenaltiesTempurate")
CASES = load_golden("sampling")
FILTER = [c for c in CASES if c["op"] == "MojoTopPFilter"]
SAMPLERS = [c for c in CASES if c["op"] in ("MojoTopKSampling", "MojoTopPSampling")]
PENALTIES = [c for c in CASES if c["op"] == "MojoApplyPenaltiesTempurate"]
REJECT = [c for c in CASES if c["op"] in ("MojoRejectSampling", "MojoJoinProbRejectSampling")]
NEG_INF = -float("inf")


def _ids(cases):
    return [pytest.param(c, id=f"{c['op'][4:]}-{i}") for i, c in enumerate(cases)]


def _golden(case):
    return getattr(G, "Torch" + case["op"][4:])(**case["ctor"]["kwargs"])


@pytest.mark.parametrize("case", _ids(FILTER))
def test_filter_golden_reproduces_the_reference_bit_for_bit(case):
    out = _golden(case).forward(*clone_tree(case["args"]))
    assert bit_equal(out, case["out"])
    logits, _, _, k = case["args"]
    assert out[0].dtype == logits.dtype and out[1].dtype == torch.int64
    assert out[0].shape == out[1].shape == logits.shape[:-1] + (min(k, logits.shape[-1]),)


@pytest.mark.parametrize("case", _ids(SAMPLERS))
def test_sampler_golden_reproduces_the_reference_distribution_and_draws_from_it(case):
    op = _golden(case)
    logits = case["args"][0]
    if case["op"] == "MojoTopKSampling":
        values, indices = G.topk_sorted(logits.float(), op.effective_k(logits.shape[-1]))
        probs = torch.softmax(values, dim=-1)
    else:
        probs, indices, _ = G.top_p_filter(logits, op.top_p, op.min_tokens_to_keep, op.rand_top_k, op.filter_value)
    assert bit_equal((probs, indices), case["out"])
    next_probs, next_tokens = op.forward(logits.clone())
    assert next_probs.dtype == torch.float32 and next_tokens.dtype == torch.int64
    assert next_probs.shape == next_tokens.shape == logits.shape[:-1] + (1,)
    where = (indices == next_tokens)
    assert bool((where.sum(-1) == 1).all())                                     # a token of the candidate set ...
    assert torch.equal(probs[where].reshape(next_probs.shape), next_probs)      # ... with its probability
    assert bool((next_probs > 0).all())


@pytest.mark.parametrize("case", _ids(PENALTIES))
def test_penalties_golden_reproduces_the_reference_bit_for_bit(case):
    args = clone_tree(case["args"])
    out = _golden(case).forward(*args)
    assert bit_equal(out, case["out"])
    if case["args"][0].dtype == torch.float32:
        assert out is args[0]                                                   # updated in place and returned
    else:
        assert out is not args[0] and torch.equal(args[0], case["args"][0]) and out.dtype == args[0].dtype


@pytest.mark.parametrize("case", _ids(REJECT))
def test_reject_golden_reproduces_the_reference_bit_for_bit(case):
    out = _golden(case).forward(*clone_tree(case["args"]), **case["kwargs"])   # reseeds, then draws on the CPU
    assert bit_equal(out, case["out"])
    # the same uniforms handed over give the same answer
    torch.manual_seed(case["kwargs"]["random_seed"])
    batch, steps = case["args"][1].shape
    u = torch.rand(batch, 1 if case["op"] == "MojoRejectSampling" else steps)
    assert bit_equal(_golden(case).forward(*clone_tree(case["args"]), uniforms=u), case["out"])


def test_ties_go_to_the_lower_index():
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-6, 7, (7, 400), generator=g).float() / 4                 # 49 distinct values over 400 columns
    for k in (1, 13, 64, 400):
        values, indices = G.topk_sorted(x, k)
        assert torch.equal(values, torch.sort(x, dim=-1, descending=True).values[:, :k])
        assert torch.equal(torch.gather(x, -1, indices), values)
        same = values[:, 1:] == values[:, :-1]
        assert bool(same.any()) or k == 1
        assert bool((indices[:, 1:] > indices[:, :-1])[same].all())             # lower indices first inside a run
        for r in range(x.shape[0]):                                             # a tie across position k keeps the lower indices
            last = values[r, -1]
            taken = indices[r][values[r] == last]
            candidates = torch.nonzero(x[r] == last).flatten()
            assert torch.equal(taken, candidates[: taken.numel()])
    tie_free = torch.randperm(500, generator=g).float().reshape(2, 250)
    assert bit_equal(G.topk_sorted(tie_free, 40), tuple(torch.topk(tie_free, 40)))


def test_fixtures_cover_what_they_must():
    assert os.path.getsize(os.path.join(GOLDEN, "sampling.pt")) < (1 << 20)
    assert {c["op"] for c in CASES} == set(OPS)
    # filter
    assert {c["args"][0].dtype for c in FILTER} == {torch.float32, torch.bfloat16, torch.float16}
    shapes = [(c["args"][0].shape[-1], c["args"][3]) for c in FILTER]
    assert any(k < v for v, k in shapes) and any(k == v for v, k in shapes) and any(k > v for v, k in shapes)
    assert any(c["args"][2] == 1 for c in FILTER) and any(c["args"][2] > 1 for c in FILTER)
    finite = [c for c in FILTER if c["ctor"]["kwargs"]["filter_value"] != NEG_INF]
    assert finite and all(torch.isfinite(torch.tensor(c["ctor"]["kwargs"]["filter_value"])) for c in finite)
    assert any(bool((c["out"][0].float() > 0).all()) for c in finite)           # removed positions keep a share
    assert any(c["args"][0].dim() == 3 for c in FILTER)
    for c in FILTER:                                                            # 16-bit rows: distinct representable values
        x = c["args"][0]
        if x.dtype != torch.float32:
            flat = x.float().reshape(-1, x.shape[-1])
            assert all(row.unique().numel() == row.numel() for row in flat)
    lone = [c for c in FILTER if "first_token_exceeds_row" in c]
    assert lone
    for c in lone:
        r = c["first_token_exceeds_row"]
        x, top_p = c["args"][0], c["args"][1]
        assert torch.softmax(x[r].float(), -1).max() > top_p
        assert c["out"][0][r, 0] == 1.0 and not c["out"][0][r, 1:].any()
    # a min_tokens_to_keep that decides: more positions kept than the running sum alone would keep
    decided = False
    for c in FILTER:
        _, top_p, keep, k = c["args"]
        if keep > 1 and c["ctor"]["kwargs"]["filter_value"] == NEG_INF:
            _, _, values = G.top_p_filter(c["args"][0], top_p, keep, k, NEG_INF)
            loose = G.nucleus(values, top_p, 1, NEG_INF)
            decided |= bool(((c["out"][0].float() > 0).sum(-1) > (loose > 0).sum(-1)).any())
    assert decided
    # samplers: the distribution and the indices, not a draw
    for c in SAMPLERS:
        probs, indices = c["out"]
        assert probs.dtype == torch.float32 and indices.dtype == torch.int64 and probs.shape == indices.shape
        assert probs.shape[-1] > 1 and torch.allclose(probs.sum(-1), torch.ones(probs.shape[:-1]), atol=1e-5)
    assert {c["op"] for c in SAMPLERS} == {"MojoTopKSampling", "MojoTopPSampling"}
    assert {c["args"][0].dim() for c in SAMPLERS} == {1, 2}
    # penalties
    assert {c["args"][0].dtype for c in PENALTIES} == {torch.float32, torch.bfloat16}
    assert {f.dtype for c in PENALTIES for f in c["args"][1] if f is not None} == {torch.int32, torch.float32}
    assert all(any(f is None for f in c["args"][1]) for c in PENALTIES)
    assert any(c["args"][5] is None for c in PENALTIES)
    assert any(c["args"][5] is not None and None in c["args"][5] for c in PENALTIES)
    for c in PENALTIES:
        _, freqs, presence, frequency, repetition, _ = c["args"]
        assert any(f is not None and (p, q, r) == (0.0, 0.0, 1.0) for f, p, q, r in zip(freqs, presence, frequency, repetition))
    # reject samplers: seeded; all accepted, first rejected, one in the middle rejected
    assert {c["op"] for c in REJECT} == {"MojoRejectSampling", "MojoJoinProbRejectSampling"}
    for c in REJECT:
        assert c["kwargs"]["random_seed"] is not None
        steps = c["args"][1].shape[1]
        tokens, accepted = c["out"]
        assert accepted.dtype == (torch.int64 if c["op"] == "MojoRejectSampling" else torch.int32)
        assert tokens.dtype == torch.int64 and torch.equal(tokens[:, :steps], c["args"][1]) and not tokens[:, steps].any()
        lens = accepted.tolist()
        assert steps in lens and 0 in lens and any(0 < v < steps for v in lens)


@pytest.mark.parametrize("name", OPS)
def test_dispatch_registers_torch_and_hip(name):
    core = getattr(mo, name)
    assert core.get_backend_impl("torch", strict=True).__name__ == "Torch" + name[4:]
    from mojo_opset_amd.backends import hip

    hip_cls = getattr(hip, "HIP" + name[4:])
    assert issubclass(hip_cls, core)
    if get_platform() == "rocm":
        assert core.get_backend_impl("hip", strict=True) is hip_cls


def test_sampling_ops_are_attributes_but_in_no_other_set():
    assert tuple(mo.SAMPLING_OPS) == OPS
    for name in OPS:
        assert name not in mo.__all__ and name not in mo.EXTENDED_OPS and name not in mo.KV_INT8_OPS and name not in mo.QUANT_MOE_OPS
        assert getattr(mo, name).__name__ == name
    assert len(mo.__all__) == len(set(mo.__all__))


def test_rebase_registers_the_six_classes_into_a_stand_in_reference():
    from mojo_opset_amd import plugin
    from mojo_opset_amd.backends import hip

    ref = types.ModuleType("stand_in_reference_sampling")
    sys.modules[ref.__name__] = ref
    try:
        def ctor(self, *args, **kwargs):
            MojoOperator.__init__(self)

        for name in OPS:
            setattr(ref, name, type(name, (MojoOperator,), {"__init__": ctor, "forward": lambda self, *a, **k: None,
                                                            "__module__": ref.__name__}))
        made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
        for name in OPS:
            cls = made[name]
            assert cls.__name__ == "HIP" + name[4:] and issubclass(cls, getattr(ref, name))
            assert cls.forward is getattr(hip, "HIP" + name[4:]).forward
            assert "__init__" not in vars(cls)
    finally:
        del sys.modules[ref.__name__]


def test_constructors_and_repr_follow_the_reference():
    op = G.TorchTopKSampling()
    assert (op.top_k, op.filter_value, op.min_tokens_to_keep, op.op_name, op.layer_idx) == (50, NEG_INF, 1, "", 0)
    assert G.TorchTopKSampling(top_k=4, min_tokens_to_keep=9).effective_k(300) == 9 and op.effective_k(20) == 20
    op = G.TorchTopPSampling()
    assert (op.top_p, op.filter_value, op.min_tokens_to_keep, op.rand_top_k) == (0.75, NEG_INF, 1, 1000)
    assert op.extra_repr() == "top_p=0.75, filter_value=-inf, min_tokens_to_keep=1, rand_top_k=1000"
    assert G.TorchTopPFilter(filter_value=-3.0).extra_repr() == "filter_value=-3.0"
    assert not list(G.TorchRejectSampling().parameters()) and not G.TorchApplyPenaltiesTempurate().state_dict()
    with pytest.raises(ValueError):
        G.TorchApplyPenaltiesTempurate()(torch.zeros(2, 4), [None], [0.0, 0.0], [0.0, 0.0], [1.0, 1.0])


def test_hip_classes_refuse_on_the_host():
    from mojo_opset_amd.backends.hip import (HIPApplyPenaltiesTempurate, HIPRejectSampling, HIPTopKSampling, HIPTopPFilter,
                                             HIPTopPSampling)
    from mojo_opset_amd.backends.hip import lib as L
    from mojo_opset_amd.backends.hip.operators import sampling as S

    assert S.MAX_K == L.load().mojo_hip_sampling_max_k() >= 1024
    wide = torch.zeros(2, 4096)
    with pytest.raises(NotImplementedError, match=str(S.MAX_K)):                # K above the cap, named in the message
        HIPTopPFilter()(wide, 0.75, 1, S.MAX_K + 1)
    with pytest.raises(NotImplementedError, match=str(S.MAX_K)):
        HIPTopPSampling(rand_top_k=2000)(wide)
    with pytest.raises(NotImplementedError, match=str(S.MAX_K)):
        HIPTopKSampling(top_k=3000)(wide)
    with pytest.raises(NotImplementedError, match=str(S.MAX_K)):
        S.sample_with_uniforms(wide, torch.zeros(2), 1500)
    with pytest.raises(NotImplementedError):
        HIPTopPFilter()(wide.double(), 0.75, 1, 10)
    for call in (lambda: HIPTopPFilter()(wide, 0.75, 1, 1000),                 # K <= cap: no CPU path, refused before device work
                 lambda: HIPTopPFilter()(torch.zeros(2, 40), 0.75, 1, 5000),    # K clamps to V first
                 lambda: HIPTopPSampling()(wide), lambda: HIPTopKSampling()(wide),
                 lambda: HIPRejectSampling()(torch.zeros(2, 3, 8), torch.zeros(2, 2, dtype=torch.long), torch.ones(2, 2)),
                 lambda: HIPApplyPenaltiesTempurate()(torch.zeros(2, 8), [None, None], [0.0, 0.0], [0.0, 0.0], [1.0, 1.0])):
        with pytest.raises(L.MojoHipError):
            call()
    pen = HIPApplyPenaltiesTempurate()
    lists = ([0.1, 0.1], [0.1, 0.1], [1.1, 1.1])
    with pytest.raises(NotImplementedError, match="one dtype"):                 # mixed frequency dtypes
        pen(torch.zeros(2, 8), [torch.zeros(8, dtype=torch.int32), torch.zeros(8)], *lists)
    with pytest.raises(NotImplementedError):
        pen(torch.zeros(2, 8), [torch.zeros(8, dtype=torch.int16), None], *lists)
    with pytest.raises(ValueError):
        pen(torch.zeros(2, 8), [None], *lists)
    with pytest.raises(TypeError):
        S.reject_with_uniforms(torch.zeros(2, 3, 8), torch.zeros(2, 2, dtype=torch.int32), torch.ones(2, 2), torch.zeros(2, 1), False)
    assert "not captured in a graph" in " ".join(HIPApplyPenaltiesTempurate.__doc__.lower().split())


def test_workspace_query_answers_without_a_gpu():
    from mojo_opset_amd.backends.hip.operators import sampling as S

    rows, vocab, k = 120, 151936, 1000
    auto = S.workspace_bytes(rows, vocab, k)
    sizes = [S.workspace_bytes(rows, vocab, k, s) for s in (1, 2, 8, 16, 32, 64)]
    assert all(b > 0 and b % 8 == 0 for b in sizes + [auto])
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]                       # grows with the slice count
    assert S.workspace_bytes(rows, vocab, k, 32) == rows * 32 * k * 8            # K composites of 8 bytes per (row, slice)
    assert S.workspace_bytes(15, 155136, 100) >= 15 * 100 * 8
    assert S.workspace_bytes(4, 40, 40, 1) == 4 * 40 * 8                         # a slice shorter than K keeps all of itself
    assert S.workspace_bytes(0, vocab, k) == 0
