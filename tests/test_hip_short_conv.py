"""GPU tests of the short-convolution ops (`SHORT_CONV_OPS`: `MojoCausalConv1dUpdateState`, `MojoCausalConv1d`) through the C ABI,
judged against the CPU goldens (tests/short_conv_golden.py, pinned to the reference by tests/test_short_conv_golden.py):

* activation ``None``: output, updated state and final state are bit-identical to the golden, signed zeros included - the
  kernels follow the golden's fp32 order with the product and the sum rounded separately;
* SiLU in 16 bits: every output within one storage ulp of fp64 SiLU of the golden's fp32 pre-activation; in fp32: bit-identical
  to `HIPSilu` applied to that pre-activation;
* residual: ``storage(y) + residual`` with ``y`` from the same call without the residual, bit for bit;
* states are copies: always bit-identical.

The shapes are the smallest at which each path can go wrong; the run length of the channel-contiguous kernel and the
switch-over of the time-contiguous forms are read from the library."""
import pytest
import torch

import short_conv_golden as G
from conftest import load_golden
from hip_utils import DEV, hip_cls, last_launch
from mojo_opset_amd.backends.hip.operators import convolution as backend

pytestmark = pytest.mark.gpu
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "fp16", "fp32"])
MANTISSA = {BF16: (7, -126), F16: (10, -14)}
PACKED_IDS = ["int32", "int64"]


def same_bits(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    as_int = torch.int32 if a.element_size() == 4 else torch.int16
    a, b = a.contiguous().view(as_int), b.contiguous().view(as_int)
    return torch.equal(a, b)


def assert_output(got, detail, activation, key="out"):
    """``got`` against the golden's detail by the rule of its activation (module docstring)."""
    got = got.detach().cpu()
    assert got.dtype == detail[key].dtype and got.shape == detail[key].shape
    if activation is None:
        assert same_bits(got, detail[key])
    elif got.dtype == F32:
        assert same_bits(got, hip_cls("MojoSilu")().forward(detail["pre"].to(DEV)))
    else:
        mant, e_min = MANTISSA[got.dtype]
        want = detail["pre"].double() * torch.sigmoid(detail["pre"].double())
        ulp = torch.pow(2.0, torch.floor(torch.log2(want.abs().clamp_min(2.0 ** e_min))) - mant)
        assert bool(((got.double() - want).abs() <= ulp).all()), float(((got.double() - want).abs() / ulp).max())


def expected_vec(dtype, dim, offset=0):
    """Elements of the widest channel vector that ``dim`` and a base ``offset`` elements into an aligned buffer allow."""
    size = torch.empty(0, dtype=dtype).element_size()
    for nbytes in (16, 8, 4):
        v = nbytes // size
        if v > 1 and dim % v == 0 and offset % v == 0:
            return v
    return 1


def tensors(g, dtype, *shapes):
    return [torch.randn(*s, generator=g).to(dtype) for s in shapes]


def run_update(hidden, state, weight, bias, activation):
    """The HIP op on device tensors (``state`` is rewritten) and the golden on their CPU copies."""
    detail = G.update_state_detail(hidden.cpu(), state.cpu(), weight.cpu(), None if bias is None else bias.cpu(), activation)
    out = hip_cls("MojoCausalConv1dUpdateState")().forward(hidden, state, weight, bias, activation)
    torch.cuda.synchronize()
    return out, detail


def run_conv(x, weight, **kw):
    cpu = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    final = cpu.pop("output_final_state", False)
    detail = G.conv1d_detail(x.cpu(), weight.cpu(), **cpu)
    out, state = hip_cls("MojoCausalConv1d")().forward(x, weight, **kw)
    torch.cuda.synchronize()
    assert (state is not None) == bool(final)
    return out, state, detail


@pytest.mark.parametrize("case", [pytest.param(c, id=f"{c['op']}-{c['label']}") for c in load_golden("short_conv")])
def test_recorded_cases(case):
    args = [a.to(DEV) if isinstance(a, torch.Tensor) else a for a in G.case_args(case)]
    if case["op"] == "MojoCausalConv1dUpdateState":
        out, detail = run_update(*args)
        assert_output(out, detail, args[4])
        assert same_bits(args[1], detail["state"]) and same_bits(args[1], case["state_after"])
        return
    kw = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in case["kwargs"].items()}
    out, state, detail = run_conv(*args, **kw)
    if kw.get("residual") is None:
        assert_output(out, detail, kw.get("activation"))
    else:
        plain = hip_cls("MojoCausalConv1d")().forward(*args, **{k: v for k, v in kw.items() if k != "residual"})[0]
        assert_output(plain, detail, kw.get("activation"), key="conv_out")
        assert same_bits(out, (plain.float() + kw["residual"].float()).to(plain.dtype))
    if state is not None:
        assert same_bits(state, detail["final_state"])


@DTYPES
@pytest.mark.parametrize("dim", [8, 24, 1000, 1001, 1004])
def test_channel_contiguous_update_on_a_transposed_view(dim, dtype):
    """The update op on ``y.transpose(1, 2)`` of a ``[B, T, D]`` tensor, as HF-style model code calls it.  D 8: one 16-byte vector
    (fp32: two); 24 and 1000: several; 1004: 8-byte vectors in 16 bits; 1001: single elements.  T in {1, W - 2, W - 1, W} and one T
    of three runs and a tail; S in {W - 1, W, 7}, so T < S (the state shifts) and T >= S both occur.  The output comes back with
    the view's strides."""
    run = backend.run_tokens()
    g = torch.Generator().manual_seed(dim)
    n = 0
    for width in (2, 3, 4):
        for seq in sorted({1, max(width - 2, 1), width - 1, width, 3 * run + 5}):
            for state_len in (width - 1, width, 7):
                act = (None, "silu", None, "swish")[n % 4]
                n += 1
                y, state, weight, bias = tensors(g, dtype, (2, seq, dim), (2, dim, state_len), (dim, width), (dim,))
                hidden, state, weight, bias = y.to(DEV).transpose(1, 2), state.to(DEV), weight.to(DEV), bias.to(DEV)
                out, detail = run_update(hidden, state, weight, bias if n % 3 else None, act)
                assert last_launch() == f"causal_conv1d:channel:vec{expected_vec(dtype, dim)}:batched", (width, seq, state_len)
                assert out.shape == hidden.shape and out.stride() == hidden.stride()
                assert_output(out, detail, act)
                assert same_bits(state, detail["state"]), (width, seq, state_len)


@DTYPES
def test_channel_contiguous_reads_a_column_slice_in_place(dtype):
    """x, the residual and the update op's view are column slices of wider buffers: a base 2 elements in (4- or 8-byte vectors),
    1 element in (single elements), 8 elements in with a row stride larger than D (16-byte vectors)."""
    g = torch.Generator().manual_seed(9)
    dim, seq = 24, 37
    wide, rwide, weight, bias, init = tensors(g, dtype, (2, seq, dim + 16), (2, seq, dim + 16), (dim, 4), (dim,), (2, dim, 3))
    wide, rwide, weight, bias, init = (t.to(DEV) for t in (wide, rwide, weight, bias, init))
    for first in (2, 1, 8):
        x, res = wide[:, :, first:first + dim], rwide[:, :, first:first + dim]
        out, state, detail = run_conv(x, weight, bias=bias, initial_state=init, output_final_state=True)
        assert last_launch() == f"causal_conv1d:channel:vec{expected_vec(dtype, dim, first)}:batched"
        assert_output(out, detail, None)
        assert same_bits(state, detail["final_state"])
        with_res = run_conv(x, weight, bias=bias, initial_state=init, residual=res)[0]
        assert same_bits(with_res, (out.float() + res.float()).to(dtype))
        conv_state = init.clone()
        upd, udetail = run_update(x.transpose(1, 2), conv_state, weight, bias, None)
        assert last_launch() == f"causal_conv1d:channel:vec{expected_vec(dtype, dim, first)}:batched"
        assert_output(upd, udetail, None)
        assert same_bits(conv_state, udetail["state"]) and same_bits(upd.transpose(1, 2), out)


@DTYPES
@pytest.mark.parametrize("cu_dtype", [torch.int32, torch.int64], ids=PACKED_IDS)
def test_packed_sequences(cu_dtype, dtype):
    """Lengths [1, 2, 3, 0, run + 1, 2 run - 1]: sequences inside one run, an empty one, one that crosses a run boundary and one
    that fills runs; with and without `initial_state`; every width; the residual rule."""
    run = backend.run_tokens()
    lengths = [1, 2, 3, 0, run + 1, 2 * run - 1]
    cu = torch.tensor([0] + torch.tensor(lengths).cumsum(0).tolist(), dtype=cu_dtype)
    g = torch.Generator().manual_seed(21)
    for n, width in enumerate((2, 3, 4)):
        act = (None, "silu", None)[n]
        x, res, weight, bias, init = tensors(g, dtype, (1, sum(lengths), 24), (1, sum(lengths), 24), (24, width), (24,), (6, 24, width - 1))
        x, res, weight, bias, init, cud = (t.to(DEV) for t in (x, res, weight, bias, init, cu))
        for state in (None, init):
            out, final, detail = run_conv(x, weight, bias=bias, initial_state=state, output_final_state=True, activation=act,
                                          cu_seqlens=cud)
            assert last_launch() == f"causal_conv1d:channel:vec{expected_vec(dtype, 24)}:packed"
            assert_output(out, detail, act)
            assert same_bits(final, detail["final_state"])
            with_res = run_conv(x, weight, bias=bias, initial_state=state, activation=act, cu_seqlens=cud, residual=res)[0]
            assert same_bits(with_res, (out.float() + res.float()).to(dtype))
        if state is not None:
            assert same_bits(final[3], init[3])                          # the empty sequence hands its state on


def test_no_tap_crosses_a_sequence_boundary():
    """Sequence k's inputs are NaN: sequence k + 1's outputs and state stay finite and equal the golden's."""
    run = backend.run_tokens()
    lengths = [1, 2, 3, 0, run + 1, 2 * run - 1]
    cu = torch.tensor([0] + torch.tensor(lengths).cumsum(0).tolist())
    g = torch.Generator().manual_seed(22)
    x, weight, init = tensors(g, BF16, (1, sum(lengths), 24), (24, 4), (6, 24, 3))
    for k in (0, 1, 2, 4):
        poisoned = x.clone()
        poisoned[0, cu[k]:cu[k + 1]] = float("nan")
        for state in (None, init):
            out, final, detail = run_conv(poisoned.to(DEV), weight.to(DEV), initial_state=None if state is None else state.to(DEV),
                                          output_final_state=True, cu_seqlens=cu.to(DEV))
            out, final = out.cpu(), final.cpu()
            nxt = k + 2 if lengths[k + 1] == 0 else k + 1
            assert bool(out[0, cu[nxt]:cu[nxt + 1]].isfinite().all()) and bool(final[nxt].isfinite().all())
            assert bool(out[0, cu[k]:cu[k + 1]].isnan().all())
            clean = torch.ones(sum(lengths), dtype=torch.bool)
            clean[cu[k]:cu[k + 1]] = False
            assert same_bits(out[0, clean], detail["out"][0, clean]) and same_bits(final[nxt], detail["final_state"][nxt])


@DTYPES
@pytest.mark.parametrize("dim", [3, 130])
def test_time_contiguous_update(dim, dtype):
    """The reference's literal ``[B, D, T]``: T in {1, 2, 7, 8, 9, 257} and both sides of the switch-over between the
    row-per-thread form and the vector form.  Dense rows of an odd T start at every misalignment, so the vector form peels
    heads and tails of every length."""
    limit = backend.row_thread_max_t()
    wide = 16 // torch.empty(0, dtype=dtype).element_size()
    g = torch.Generator().manual_seed(dim + 1)
    n = 0
    for width in (2, 3, 4):
        for seq in sorted({1, 2, 7, 8, 9, 257, limit, limit + 1}):
            state_len = (width - 1, width, 7)[n % 3]
            act = (None, "silu", None, "swish")[n % 4]
            n += 1
            hidden, state, weight, bias = (t.to(DEV) for t in tensors(g, dtype, (3, dim, seq), (3, dim, state_len), (dim, width), (dim,)))
            out, detail = run_update(hidden, state, weight, bias if n % 3 else None, act)
            assert last_launch() == ("causal_conv1d:time:row" if seq <= limit else f"causal_conv1d:time:vec{wide}"), seq
            assert out.is_contiguous()
            assert_output(out, detail, act)
            assert same_bits(state, detail["state"]), (width, seq, state_len)


@DTYPES
def test_time_contiguous_rows_misaligned_by_one_element(dtype):
    """x starts one element into its buffer and its rows lie T + 8 apart: the rows of x and of the dense output are misaligned
    differently, so long rows go by single elements; short rows take the row form as ever.  The function op on a time-contiguous
    ``[B, T, D]`` view takes the same kernels, with the residual."""
    limit = backend.row_thread_max_t()
    g = torch.Generator().manual_seed(31)
    for seq in (limit, 61):
        buf, state, weight, bias, res = tensors(g, dtype, (2, 5, seq + 8), (2, 5, 3), (5, 4), (5,), (2, seq, 5))
        buf, state, weight, bias, res = (t.to(DEV) for t in (buf, state, weight, bias, res))
        hidden = buf[:, :, 1:1 + seq]
        tag = "causal_conv1d:time:row" if seq <= limit else "causal_conv1d:time:vec1"
        before = state.clone()
        out, detail = run_update(hidden, state, weight, bias, None)
        assert last_launch() == tag
        assert_output(out, detail, None)
        assert same_bits(state, detail["state"])
        x = hidden.transpose(1, 2)                                           # [B, T, D] with stride(T) == 1
        conv, final, cdetail = run_conv(x, weight, bias=bias, initial_state=before, output_final_state=True, residual=res)
        assert last_launch() == tag and conv.shape == x.shape
        assert same_bits(conv, cdetail["out"]) and same_bits(final, cdetail["final_state"])
        assert same_bits(conv, (out.transpose(1, 2).float() + res.float()).to(dtype))


@DTYPES
def test_in_place_state_with_t_spanning_several_workgroups(dtype):
    """The state is input and output of one launch.  Channel form: 8 runs x 125 vectors per sequence (8 workgroups); time form:
    rows of 4099 elements, two workgroups per row.  The first W - 1 outputs (which read the old state) and the new state are
    both checked, as is everything else."""
    run = backend.run_tokens()
    g = torch.Generator().manual_seed(41)
    for layout, dim, seq in (("channel", 1000, 8 * run), ("time", 6, 4099)):
        for width, state_len in ((4, 3), (3, 7), (2, 2)):
            y, state, weight = tensors(g, dtype, (2, seq, dim) if layout == "channel" else (2, dim, seq), (2, dim, state_len), (dim, width))
            hidden = y.to(DEV).transpose(1, 2) if layout == "channel" else y.to(DEV)
            state, weight = state.to(DEV), weight.to(DEV)
            out, detail = run_update(hidden, state, weight, None, None)
            assert last_launch().startswith(f"causal_conv1d:{layout}:vec")
            assert same_bits(out[:, :, :width - 1], detail["out"][:, :, :width - 1])
            assert same_bits(state, detail["state"]) and same_bits(out, detail["out"])


@pytest.mark.parametrize("layout", ["time", "channel"])
def test_decode_step_replays_in_a_graph(layout):
    """B 3, D 130, T 1 captured once and replayed three times on static buffers: three golden steps, the state carried along."""
    g = torch.Generator().manual_seed(51)
    steps = tensors(g, BF16, (3, 130, 1), (3, 130, 1), (3, 130, 1))
    state0, weight, bias = tensors(g, BF16, (3, 130, 3), (130, 4), (130,))
    static = torch.zeros(3, 130, 1, dtype=BF16, device=DEV) if layout == "time" else \
        torch.zeros(3, 1, 130, dtype=BF16, device=DEV).transpose(1, 2)
    state, weight_d, bias_d = torch.zeros_like(state0, device=DEV), weight.to(DEV), bias.to(DEV)
    op = hip_cls("MojoCausalConv1dUpdateState")()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        op.forward(static, state, weight_d, bias_d, "silu")                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert last_launch() == ("causal_conv1d:time:row" if layout == "time" else "causal_conv1d:channel:vec2:batched")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = op.forward(static, state, weight_d, bias_d, "silu")
    state.copy_(state0)
    cpu_state = state0.clone()
    for hidden in steps:
        static.copy_(hidden)
        graph.replay()
        torch.cuda.synchronize()
        detail = G.update_state_detail(hidden, cpu_state, weight, bias, "silu")
        cpu_state = detail["state"]
        assert_output(out, detail, "silu")
        assert same_bits(state, cpu_state)
