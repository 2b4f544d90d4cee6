"""Write tests/golden/sampling.pt: reference outputs of the sampling ops (authoring machine only).

Usage: python oracle/make_sampling_golden.py [reference root]   (default: MOJO_REFERENCE_ROOT, else /root/reference; nothing else reads it)

The outputs come from the reference's own ``torch`` backends of the six classes of `mojo_opset/core/operators/sampling.py`,
built on CPU.  Each case records the constructor keywords, the inputs and the output; tests/test_sampling_golden.py pins
oracle/sampling.py to them bit for bit and tests/test_hip_sampling.py runs the hip backend on them.

* The reference selects with ``torch.topk``, which leaves the order among equal values open, so every recorded top-k input is
  asserted tie-free in its top K + 1: the recorded indices are then unambiguous.  The 16-bit rows are permutations of distinct
  representable values.
* A sampler's output is a random draw.  What is recorded instead is what the reference hands to ``torch.multinomial`` (its
  ``final_probs_dist``) and the indices of its ``torch.topk``: both calls are observed while the reference runs.
* The reject samplers are recorded with a seed: on the CPU generator the reference is reproducible.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEG_INF = -float("inf")


def assert_tie_free(logits, k):
    x = logits.float().reshape(-1, logits.shape[-1])
    top = torch.sort(x, dim=-1, descending=True).values[:, : min(k + 1, x.shape[-1])]
    assert bool((top[:, 1:] < top[:, :-1]).all()), "a recorded top-k input has a tie in its top K + 1"


def distinct_rows(g, shape, dtype, step):
    """Rows that are permutations of ``(i - V / 2) * step``: distinct and exactly representable in ``dtype``."""
    vocab = shape[-1]
    rows = int(torch.tensor(shape[:-1]).prod()) if len(shape) > 1 else 1
    base = (torch.arange(vocab, dtype=torch.float32) - vocab // 2) * step
    out = torch.stack([base[torch.randperm(vocab, generator=g)] for _ in range(rows)]).reshape(shape).to(dtype)
    assert torch.equal(out.float().reshape(rows, vocab).sort(dim=-1).values, base.sort().values.expand(rows, vocab))
    return out


class Observed:
    """Records the arguments of ``torch.multinomial`` and the result of ``torch.topk`` while the reference runs."""

    def __enter__(self):
        self.multinomial, self.topk = torch.multinomial, torch.topk
        self.probs = self.indices = None

        def multinomial(probs, num_samples=1, **kw):
            self.probs = probs.clone()
            return self.multinomial(probs, num_samples=num_samples, **kw)

        def topk(x, k, *a, **kw):
            out = self.topk(x, k, *a, **kw)
            self.indices = out[1].clone()
            return out

        torch.multinomial, torch.topk = multinomial, topk
        return self

    def __exit__(self, *exc):
        torch.multinomial, torch.topk = self.multinomial, self.topk


def main(reference_root):
    sys.path.insert(0, reference_root)
    import mojo_opset as ref

    g = torch.Generator().manual_seed(4171)
    cases = []

    def build(op, kwargs):
        return getattr(ref, op)._registry.get("torch")(**kwargs)

    def record(op, kwargs, args, call_kwargs=None, **extra):
        call_kwargs = call_kwargs or {}
        with torch.no_grad():
            out = build(op, kwargs)(*[a.clone() if isinstance(a, torch.Tensor) else a for a in args], **call_kwargs)
        cases.append({"op": op, "ctor": {"kwargs": kwargs}, "state": {}, "args": tuple(args), "kwargs": call_kwargs, "out": out, **extra})

    # ---- MojoTopPFilter: args (logits, top_p, min_tokens_to_keep, rand_top_k) ----
    def filter_case(logits, top_p, keep, k, filter_value=NEG_INF, **extra):
        assert_tie_free(logits, min(k, logits.shape[-1]))
        record("MojoTopPFilter", {"filter_value": filter_value}, [logits, top_p, keep, k], **extra)

    filter_case(torch.randn(5, 300, generator=g) * 2, 0.75, 1, 50)                                   # fp32, K < V
    filter_case(distinct_rows(g, (4, 200), torch.bfloat16, 1 / 16), 0.7, 1, 64)                       # bf16, K < V
    filter_case(distinct_rows(g, (3, 64), torch.float16, 1 / 8), 0.8, 1, 64)                          # fp16, K == V
    filter_case(torch.randn(3, 40, generator=g) * 3, 0.6, 1, 1000)                                    # rand_top_k > V
    filter_case(torch.randn(4, 256, generator=g) * 4, 0.3, 3, 32)                                     # min_tokens_to_keep > 1 decides
    filter_case(torch.randn(4, 256, generator=g) * 2, 0.5, 1, 48, filter_value=-3.0)                  # finite filter value
    filter_case(torch.randn(4, 256, generator=g) * 2, 0.5, 4, 48, filter_value=1.5)                   # ... above some kept logits
    filter_case(torch.randn(2, 3, 128, generator=g) * 2, 0.75, 1, 40)                                 # 3-D
    peaked = torch.randn(3, 160, generator=g)
    peaked[1, 77] = 12.0                                                                              # one token above top_p alone
    filter_case(peaked, 0.75, 1, 20, first_token_exceeds_row=1)
    filter_case(distinct_rows(g, (2, 2, 96), torch.bfloat16, 1 / 8), 0.9, 2, 96, filter_value=-2.0)   # bf16, 3-D, K == V, finite

    # ---- samplers: the recorded output is (final_probs_dist, indices), observed inside the reference ----
    def sampler_case(op, kwargs, logits, k):
        assert_tie_free(logits, k)
        with Observed() as seen, torch.no_grad():
            probs, tokens = build(op, kwargs)(logits.clone())
        assert probs.shape == tokens.shape == logits.shape[:-1] + (1,) and tokens.dtype == torch.int64 and probs.dtype == torch.float32
        cases.append({"op": op, "ctor": {"kwargs": kwargs}, "state": {}, "args": (logits,), "kwargs": {},
                      "out": (seen.probs, seen.indices)})

    sampler_case("MojoTopKSampling", {"top_k": 20}, torch.randn(6, 500, generator=g) * 2, 20)
    sampler_case("MojoTopKSampling", {"top_k": 4, "min_tokens_to_keep": 9}, torch.randn(300, generator=g) * 2, 9)   # 1-D, K raised
    sampler_case("MojoTopKSampling", {"top_k": 50}, distinct_rows(g, (3, 32), torch.bfloat16, 1 / 4), 32)           # top_k > V
    sampler_case("MojoTopPSampling", {"top_p": 0.6, "rand_top_k": 100}, torch.randn(6, 500, generator=g) * 2, 100)
    sampler_case("MojoTopPSampling", {"top_p": 0.4, "min_tokens_to_keep": 5, "rand_top_k": 64, "filter_value": -5.0},
                 distinct_rows(g, (4, 128), torch.float16, 1 / 8), 64)

    # ---- MojoApplyPenaltiesTempurate ----
    def freq_row(vocab, dtype):
        f = torch.randint(0, 4, (vocab,), generator=g) * (torch.rand(vocab, generator=g) < 0.3)
        return f.to(dtype)

    rows, vocab = 5, 96
    for dtype, fdtype, temps in [(torch.float32, torch.int32, [0.7, None, 1.3, 1.0, 0.5]),
                                 (torch.bfloat16, torch.float32, None),
                                 (torch.float32, torch.float32, [None, 2.0, None, 0.9, 1.1]),
                                 (torch.bfloat16, torch.int32, [0.8, 0.8, None, 1.5, 1.0])]:
        logits = (torch.randn(rows, vocab, generator=g) * 3).to(dtype)
        freqs = [freq_row(vocab, fdtype), None, freq_row(vocab, fdtype), freq_row(vocab, fdtype), None]
        record("MojoApplyPenaltiesTempurate", {},
               [logits, freqs, [0.5, 0.2, 0.0, 0.0, 0.3], [0.1, 0.4, 0.0, 0.25, 0.0], [1.2, 1.1, 1.0, 1.0, 0.8], temps])
    # (row 2: every penalty at its neutral value with a frequency row present)

    # ---- reject samplers, seeded ----
    batch, steps, vocab = 6, 3, 32
    target = torch.softmax(torch.randn(batch, steps + 1, vocab, generator=g), dim=-1)
    draft_tokens = torch.randint(0, vocab, (batch, steps), generator=g)
    picked = torch.gather(target[:, :steps], -1, draft_tokens.unsqueeze(-1)).squeeze(-1)
    ratio = torch.tensor([[2.0, 2.0, 2.0],            # every token accepted
                          [1e-6, 2.0, 2.0],           # the first rejected
                          [2.0, 1e-6, 2.0],           # one in the middle rejected
                          [2.0, 2.0, 1e-6],           # the last rejected
                          [0.5, 0.5, 0.5],            # decided by the draw
                          [0.9, 0.2, 0.7]])
    draft_probs = picked / ratio
    for seed in (7, 8):
        for op in ("MojoRejectSampling", "MojoJoinProbRejectSampling"):
            record(op, {}, [target, draft_tokens, draft_probs], {"random_seed": seed})

    path = os.path.join(ROOT, "tests", "golden", "sampling.pt")
    torch.save({"cases": cases}, path)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")
    for c in cases:
        if "Reject" in c["op"]:
            print(c["op"], c["kwargs"], c["out"][1].tolist())


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MOJO_REFERENCE_ROOT", "/root/reference"))
