"""The sampling selection on the MI355X against the pin of tests/sampling_pin.py: on every constructed case and
every slice count the indices are the golden's exactly, the probabilities are judged as in tests/test_hip_sampling.py with
NO undecidable row allowed, every slice count gives the bits of ``slices=0``, and the launch tag names the geometry the host
mirror computed.  tests/test_sampling_pin_golden.py holds the cases, the mirror and the judge to their claims without a GPU."""
import functools

import pytest
import torch

import mojo_opset_amd as mo
import sampling_pin as P
from conftest import bit_equal
from sampling_judge import Judged, _cdf_targets, _check_draw

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = list(P.CASES)
SAMPLED = [n for n in NAMES if n.split("-")[0] in ("constant", "two_level", "minus_inf")]
PUBLIC = "two_level-k64-bf16"


def _S():
    from mojo_opset_amd.backends.hip.operators import sampling as S

    return S


def _last_launch():
    from mojo_opset_amd.backends.hip import lib as L

    return L.last_launch()


def _filter(logits, c, slices):
    probs, indices = _S().top_p_filter(logits, c.top_p, c.keep, c.k, c.filter_value, slices)
    torch.cuda.synchronize()
    return probs.cpu(), indices.cpu(), _last_launch()


@functools.lru_cache(maxsize=None)
def _base(name):
    """The ``slices=0`` result of a case, launched once."""
    c = P.get_case(name)
    return _filter(c.logits.to(DEV), c, 0)


@pytest.mark.parametrize("slices", P.SLICES)
@pytest.mark.parametrize("name", NAMES)
def test_filter_on_every_case_and_slice_count(name, slices):
    c = P.get_case(name)
    probs, indices, tag = _base(name) if slices == 0 else _filter(c.logits.to(DEV), c, slices)
    geo = P.geometry(c.rows, c.vocab, c.k, slices)
    print(f"{name} slices={slices}: {tag}; {c.note['text']}")
    assert tag == f"sampling:filter:top_p:{geo.tag}"
    assert probs.shape == indices.shape == (c.rows, c.k)
    assert torch.equal(indices, c.indices), f"{name} slices={slices}: indices differ from the golden's"
    P.judge_filter(name, probs, indices, f"{name} slices={slices}")
    assert bit_equal((probs, indices), _base(name)[:2]), f"{name}: slices={slices} differs from slices=0"


@pytest.mark.parametrize("dtype", P.DTYPES, ids=lambda d: P.SHORT[d])
@pytest.mark.parametrize("stem", P.MISALIGNED)
def test_a_misaligned_base_takes_the_narrow_loop_and_gives_the_same_bits(stem, dtype):
    name = f"{stem}-{P.SHORT[dtype]}"
    c = P.get_case(name)
    assert c.vocab % 8 == 0
    flat = torch.zeros(c.rows * c.vocab + 16, dtype=dtype, device=DEV)
    moved = flat[1: 1 + c.rows * c.vocab].view(c.rows, c.vocab)
    moved.copy_(c.logits)
    assert moved.is_contiguous() and moved.data_ptr() % 16 != 0 and flat.data_ptr() % 16 == 0
    for slices in (0, 8):
        probs, indices, tag = _filter(moved, c, slices)
        assert tag == f"sampling:filter:top_p:{P.geometry(c.rows, c.vocab, c.k, slices).tag}"
        assert bit_equal((probs, indices), _base(name)[:2]), f"{name} slices={slices}"
    P.judge_filter(name, probs, indices, f"{name} misaligned")


def _positions(k):
    """Every position for K <= 64, else 64 of them with both ends."""
    return torch.arange(k) if k <= 64 else torch.unique(torch.cat([torch.linspace(0, k - 1, 62).long(), torch.tensor([1, k - 2])]))


@pytest.mark.parametrize("name,row", [(n, r) for n in SAMPLED for r in range(1 if "wide" in n else 3)])
def test_top_k_form_picks_the_position_its_uniform_names(name, row):
    c = P.get_case(name)
    assert c.rows == (1 if "wide" in name else 3)
    judged = Judged(c.logits[row:row + 1], 2.0, 1, c.k, P.NEG_INF)               # a top_p no running sum reaches: nothing removed
    assert int(judged.kept[0]) == c.k and torch.equal(judged.indices[0], c.indices[row])
    p = judged.ref64[0]
    cdf = p.cumsum(-1) / p.sum()
    lower = torch.cat([torch.zeros(1, dtype=torch.float64), cdf[:-1]])
    pos = _positions(c.k)
    pos = pos[p[pos] > 0]                                                       # (-inf logits have no interval)
    if bool((c.values[row] == c.values[row, 0]).all()):
        u = ((pos.double() + 0.5) / c.k).float()                                # all probabilities equal: the middle of slot j
    else:
        u = ((lower[pos] + cdf[pos]) / 2).float()
    assert float((cdf[pos] - lower[pos]).min()) >= max(judged.delta, 1e-6)      # every interval far wider than fp32 can blur
    logits = c.logits[row].to(DEV).expand(pos.numel(), c.vocab)
    probs, tokens = _S().sample_with_uniforms(logits, u.to(DEV), c.k, top_p=None)
    assert _last_launch() == f"sampling:sample:top_k:{P.geometry(pos.numel(), c.vocab, c.k, 0).tag}"
    assert probs.shape == tokens.shape == (pos.numel(), 1) and probs.dtype == torch.float32 and tokens.dtype == torch.int64
    assert torch.equal(tokens.cpu()[:, 0], c.indices[row, pos]), f"{name} row {row}"
    err = float(((probs.cpu()[:, 0].double() - p[pos]).abs() / p[pos]).max())
    print(f"{name} row {row}: {pos.numel()} uniforms, relative error of the returned probability {err:.3e} (bound {judged.tol:.3e})")
    assert err <= judged.tol


@pytest.mark.parametrize("name", SAMPLED)
def test_top_p_form_agrees_with_the_filter_form(name):
    S = _S()
    c, judged = P.get_case(name), P.judged_of(name)
    assert not bool(judged.undecidable.any())
    base_probs, base_indices, _ = _base(name)
    dev_logits = c.logits.to(DEV)
    kw = dict(top_p=c.top_p, min_tokens_to_keep=c.keep, filter_value=c.filter_value)
    g = torch.Generator().manual_seed(len(name))

    def agrees(probs, tokens, what):
        """The picked token is indices[pos] with probs[pos] of the filter form (to the bit for fp32; rounded for 16-bit)."""
        where = base_indices == tokens.cpu()
        assert bool((where.sum(-1) == 1).all()), what
        filtered = base_probs[where]
        assert torch.equal(probs.cpu()[:, 0].to(c.dtype), filtered), what
        return where.float().argmax(-1)

    for what, target, u, width in _cdf_targets(judged, c.rows, g):
        assert float(width.min()) >= max(judged.delta, 1e-6), what
        probs, tokens = S.sample_with_uniforms(dev_logits, u.to(DEV), c.k, **kw)
        assert _last_launch() == f"sampling:sample:top_p:{P.geometry(c.rows, c.vocab, c.k, 0).tag}"
        assert torch.equal(tokens.cpu()[:, 0], judged.indices.gather(-1, target[:, None])[:, 0]), what
        assert torch.equal(agrees(probs, tokens, what), target), what
        want = judged.ref64.gather(-1, target[:, None])[:, 0]
        err = float(((probs.cpu()[:, 0].double() - want).abs() / want).max())
        print(f"{name} {what}: relative error of the returned probability {err:.3e} (bound {judged.tol:.3e})")
        assert err <= judged.tol
    probs, tokens = S.sample_with_uniforms(dev_logits, torch.zeros(c.rows, device=DEV), c.k, **kw)
    assert torch.equal(tokens.cpu()[:, 0], judged.indices[:, 0])                # u = 0: the first token
    agrees(probs, tokens, "u = 0")
    top = torch.full((c.rows,), float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))), device=DEV)
    probs, tokens = S.sample_with_uniforms(dev_logits, top, c.k, **kw)
    pos = agrees(probs, tokens, "u just under 1")
    assert bool((probs > 0).all())
    if c.filter_value == P.NEG_INF:
        assert bool((pos < judged.kept).all())                                  # never a removed token


def test_public_classes_on_a_two_level_case():
    c, judged = P.get_case(PUBLIC), P.judged_of(PUBLIC)
    dev_logits = c.logits.to(DEV)
    hip = lambda cls, **kw: getattr(mo, cls).get_backend_impl("hip", strict=True)(**kw)   # noqa: E731
    probs, indices = hip("MojoTopPFilter", filter_value=c.filter_value)(dev_logits, c.top_p, c.keep, c.k)
    P.judge_filter(PUBLIC, probs, indices, "MojoTopPFilter")
    assert bit_equal((probs, indices), _base(PUBLIC)[:2])
    torch.manual_seed(5)
    probs, tokens = hip("MojoTopPSampling", top_p=c.top_p, rand_top_k=c.k, min_tokens_to_keep=c.keep)(dev_logits)
    assert probs.shape == tokens.shape == (c.rows, 1) and probs.dtype == torch.float32 and tokens.dtype == torch.int64
    _check_draw(judged, probs, tokens, "MojoTopPSampling")
    everything = Judged(c.logits, 2.0, 1, c.k, P.NEG_INF)
    assert torch.equal(everything.indices, c.indices)
    probs, tokens = hip("MojoTopKSampling", top_k=c.k)(dev_logits)
    _check_draw(everything, probs, tokens, "MojoTopKSampling")
