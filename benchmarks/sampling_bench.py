"""Sampling benchmark (standalone; not part of bench.py): python benchmarks/sampling_bench.py

The hip operators next to the same composition of torch operators on the device — the golden module
(oracle/sampling.py) on GPU tensors, which is what an accelerated backend without a selection kernel runs: a sort of the
whole row, two softmaxes, a cumulative sum, a multinomial draw.  The two legs are alternated in one process, five medians per
leg (their spread is reported):

* top-k sampling (120, 151936) K 20 and (18, 155136) K 100;
* top-p filter (120, 151936) K 1000, (15, 155136) K 100 and (64, 128256) K 1000, fp32 and bf16;
* top-p sampling (64, 128256) K 1000;
* penalties and temperature (20, 151936), about 5 % non-zero frequencies.

Both legs are timed eagerly with HIP events (the ratio compares like with like; the penalties operator is host-driven by its
API anyway).  The hip leg of the selection cases is timed by graph replay as well (``us_graph``: launch overhead amortised,
what a serving loop sees); the torch composition is not replayed from a graph here.  Bytes are ALGORITHMIC: rows x V x
element size, the one read of the logits (the penalties also write them and read the int32 frequency rows).
MOJO_BENCH_ONLY=<substring> runs one case.  One JSON object."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle.sampling as G  # noqa: E402
from benchmarks.extras import HBM_PEAK_GBS, _time, _time_graph, _want, hip  # noqa: E402

LEGS = 5


def legs(f_hip, f_torch, timer):
    t_hip, t_torch = [], []
    for _ in range(LEGS):                                      # alternated legs
        t_hip.append(timer(f_hip))
        t_torch.append(timer(f_torch))
    return t_hip, t_torch


def report(t_hip, t_torch, nbytes, timer_name):
    m_hip, m_torch = statistics.median(t_hip), statistics.median(t_torch)
    spread = max(max(t_hip) - min(t_hip), max(t_torch) - min(t_torch))
    return {
        "hip": {"us": m_hip * 1e6, "us_legs": [t * 1e6 for t in t_hip], "spread_us": (max(t_hip) - min(t_hip)) * 1e6,
                "GB/s": nbytes / m_hip / 1e9, "frac_of_hbm_peak": nbytes / m_hip / 1e9 / HBM_PEAK_GBS},
        "torch": {"us": m_torch * 1e6, "us_legs": [t * 1e6 for t in t_torch], "spread_us": (max(t_torch) - min(t_torch)) * 1e6},
        "bytes": nbytes, "hip_over_torch_time": m_hip / m_torch, "timer": timer_name,
        "faster_by_more_than_the_spread": (m_torch - m_hip) > spread,
    }


def selection_case(device, op, kwargs, call_args, rows, vocab, dtype, seed):
    torch.manual_seed(seed)
    logits = torch.randn(rows, vocab, device=device).to(dtype)
    mine = hip(op)(**kwargs)
    theirs = getattr(G, "Torch" + op[4:])(**kwargs)
    t_hip, t_torch = legs(lambda: mine(logits, *call_args), lambda: theirs(logits, *call_args), lambda f: _time(f, 10, 2))
    nbytes = rows * vocab * logits.element_size()
    res = report(t_hip, t_torch, nbytes, "hip events, eager")
    t_graph = [_time_graph(lambda: mine(logits, *call_args), reps=5, replays=3) for _ in range(LEGS)]
    m = statistics.median(t_graph)
    res["hip"].update({"us_graph": m * 1e6, "us_graph_legs": [t * 1e6 for t in t_graph], "graph_GB/s": nbytes / m / 1e9,
                       "graph_frac_of_hbm_peak": nbytes / m / 1e9 / HBM_PEAK_GBS})
    return res


def bench_selection(device):
    cases = {
        "top_k_sampling_120x151936_K20_fp32": ("MojoTopKSampling", {"top_k": 20}, (), 120, 151936, torch.float32),
        "top_k_sampling_18x155136_K100_fp32": ("MojoTopKSampling", {"top_k": 100}, (), 18, 155136, torch.float32),
        "top_p_sampling_64x128256_K1000_fp32": ("MojoTopPSampling", {"top_p": 0.75, "rand_top_k": 1000}, (), 64, 128256, torch.float32),
    }
    for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        cases[f"top_p_filter_120x151936_K1000_{tag}"] = ("MojoTopPFilter", {}, (0.75, 1, 1000), 120, 151936, dtype)
        cases[f"top_p_filter_15x155136_K100_{tag}"] = ("MojoTopPFilter", {}, (0.75, 1, 100), 15, 155136, dtype)
        cases[f"top_p_filter_64x128256_K1000_{tag}"] = ("MojoTopPFilter", {}, (0.75, 1, 1000), 64, 128256, dtype)
    out = {}
    for i, (name, (op, kwargs, call_args, rows, vocab, dtype)) in enumerate(cases.items()):
        if _want(name):
            out[name] = selection_case(device, op, kwargs, call_args, rows, vocab, dtype, 20261017 + i)
            torch.cuda.empty_cache()
    return out


def bench_penalties(device):
    name = "penalties_20x151936_fp32"
    if not _want(name):
        return {}
    rows, vocab = 20, 151936
    torch.manual_seed(20261101)
    logits = torch.randn(rows, vocab, device=device)
    freqs = [None if i % 5 == 4 else (torch.randint(1, 6, (vocab,), device=device) * (torch.rand(vocab, device=device) < 0.05)).int()
             for i in range(rows)]
    lists = ([0.1 + 0.01 * i for i in range(rows)], [0.05 + 0.01 * i for i in range(rows)], [1.05 + 0.01 * i for i in range(rows)],
             [0.7 + 0.02 * i for i in range(rows)])
    mine, theirs = hip("MojoApplyPenaltiesTempurate")(), G.TorchApplyPenaltiesTempurate()
    # (fp32 logits are updated in place, and repeated penalties overflow: both legs work on a fresh copy, whose 24 MB of
    # traffic is in both times and not in the bytes)
    t_hip, t_torch = legs(lambda: mine(logits.clone(), freqs, *lists), lambda: theirs(logits.clone(), freqs, *lists),
                          lambda f: _time(f, 10, 2))
    with_freq = sum(f is not None for f in freqs)
    return {name: report(t_hip, t_torch, 2 * rows * vocab * 4 + with_freq * vocab * 4, "hip events, eager")}


if __name__ == "__main__":
    dev = torch.device("cuda", 0)
    print(json.dumps({"sampling_selection": bench_selection(dev), "sampling_penalties": bench_penalties(dev)}))
