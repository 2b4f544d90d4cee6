"""The input-embedding ops (`EMBEDDING_OPS`) benchmark (standalone; not part of bench.py):
python -m benchmarks.embedding_bench [--out profiles/embedding_bench.json]

Legs, bf16, HIP events:

  gather_8192x4096            8192 distinct random rows of a 151 936 x 4096 table (`HIPEmbedding`)
  nf4_gather_8192x192_g64     the same count from a 2^20 x 192 packed-NF4 table, group_size 64 (`HIPNF4DequantEmbedding`)
  oe_<T>_<dense|nf4>          the reference's over-encoding perf shape: vocabulary 10 086, twelve n-gram vocabularies 10086 + 2^i,
                              grams 2 .. 7 twice, dims 1536 / 192; T = 128 packed as 2 x 64 (prefill), T = 128 as [128, 1] (decode)
                              and T = 8192 packed as 4 x 2048; dense and NF4 (group_size 64) mega tables

Per leg, in one process.  Gathers: ``hip`` the op, ``sibling`` `HIPSilu` on a ``[T, D]`` tensor of the output's dtype (a streaming
kernel: reads and writes every byte once), ``torch`` the torch composition.  Over-encoding: ``concat`` the fused launch
(`over_encoding_concat`), judged against the plain gather of THIS run scaled by bytes; ``hip`` the layer, against ``gemm_alone``
(the existing GEMM on a precomputed concatenation) plus the concatenation's allowed time, and against ``torch`` (`index_select`,
`cat`, `F.linear` on precomputed n-gram ids; for NF4 the dequantisation of the selected rows as torch calls).

Every figure is the median of 5 timed regions after warm-up (min and max beside it).  Calls of a few microseconds of device work (the
NF4 gather and the T = 128 legs, ``"timing": "graph"``) are timed as replays of a captured graph of 20 calls, for every column alike:
an eager loop there measures the Python shim, not the kernels.  Judged as benchmarks/vision_tower_bench.py
judges: an op may take its sibling's time scaled by bytes read plus bytes written, plus the sibling's own min-to-max spread in this
run, plus 5 % of the sibling's median (``allowed_us``, ``hip_within_margin``).  One JSON object."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.extras import _hbm, _time, _time_graph, _want, hip  # noqa: E402
from mojo_opset_amd.backends.hip.operators.embedding import over_encoding_concat  # noqa: E402
from mojo_opset_amd.backends.hip.operators.gemm import dense_gemm  # noqa: E402

BF16 = torch.bfloat16
VOCAB, ORI, OE = 10086, 1536, 192
SIZES = [VOCAB + 2 ** i for i in range(12)]
GRAMS = [i for i in range(2, 8) for _ in range(2)]
WIDTH = ORI + len(SIZES) * OE


def _allowed(sibling, scale):
    spread = sibling["us_max"] - sibling["us_min"]
    return (sibling["us"] + spread + 0.05 * sibling["us"]) * scale


def _judge(res, key, nbytes, sibling, sibling_bytes):
    res["bytes"], res["sibling_bytes"] = nbytes, sibling_bytes
    res["allowed_us"] = _allowed(sibling, nbytes / sibling_bytes)
    res["hip_minus_sibling_us"] = res[key]["us"] - sibling["us"] * nbytes / sibling_bytes
    res["hip_within_margin"] = res[key]["us"] <= res["allowed_us"]
    return res


def _nf4_table(rows, dim, group_size, device):
    q = torch.randint(-128, 128, (rows, dim // 2), dtype=torch.int8, device=device)
    return q, torch.randn(rows, dim // group_size, device=device), torch.randn(rows, dim // group_size, device=device)


def _torch_nf4_rows(q, scale, mean, group_size, codebook, rows, dtype):
    """The reference's dequantisation of the selected rows, as torch calls."""
    bits = q.index_select(0, rows).view(torch.uint8)
    nib = torch.stack((bits & 15, bits >> 4), dim=-1).reshape(rows.numel(), -1, group_size).long()
    levels = codebook[nib.reshape(-1)].reshape(nib.shape).float()
    s, m = scale.index_select(0, rows).unsqueeze(-1), mean.index_select(0, rows).unsqueeze(-1)
    return (levels * s + m).reshape(rows.numel(), -1).to(dtype)


def gather_cases(device, out):
    silu = hip("MojoSilu")()
    tokens = 8192
    plain = None
    if _want("gather_8192x4096") or _want("oe_"):
        op = hip("MojoEmbedding")(151936, 4096, device=device, dtype=BF16)
        ids = torch.randperm(151936, device=device)[:tokens]
        x = torch.randn(tokens, 4096, device=device, dtype=BF16)
        nbytes = 2 * tokens * 4096 * 2 + ids.numel() * 8
        sib_bytes = 2 * tokens * 4096 * 2
        weight = op.weight.detach()
        res = {"hip": _hbm(_time(lambda: op(ids)), nbytes), "sibling": _hbm(_time(lambda: silu(x)), sib_bytes),
               "torch": _hbm(_time(lambda: F.embedding(ids, weight)), nbytes)}
        out["gather_8192x4096"] = _judge(res, "hip", nbytes, res["sibling"], sib_bytes)
        plain = (res["hip"], nbytes)
        del op, x, weight
        torch.cuda.empty_cache()
    if _want("nf4_gather_8192x192_g64"):
        rows, dim, gs = 2 ** 20, 192, 64
        q, scale, mean = _nf4_table(rows, dim, gs, device)
        op = hip("MojoNF4DequantEmbedding")(q, scale, mean, group_size=gs, output_dtype=BF16)
        ids = torch.randperm(rows, device=device)[:tokens]
        x = torch.randn(tokens, dim, device=device, dtype=BF16)
        nbytes = tokens * (dim // 2 + 2 * 4 * (dim // gs) + dim * 2 + 8)
        sib_bytes = 2 * tokens * dim * 2
        codebook = op.codebook.detach()
        res = {"hip": _hbm(_time_graph(lambda: op(ids)), nbytes), "sibling": _hbm(_time_graph(lambda: silu(x)), sib_bytes),
               "torch": _hbm(_time_graph(lambda: _torch_nf4_rows(q, scale, mean, gs, codebook, ids, BF16)), nbytes), "timing": "graph"}
        out["nf4_gather_8192x192_g64"] = _judge(res, "hip", nbytes, res["sibling"], sib_bytes)
        del op, q, scale, mean, x
        torch.cuda.empty_cache()
    return plain


def over_encoding_cases(device, out, plain):
    ngram = hip("MojoOverEncodingNGram")(VOCAB, SIZES, GRAMS).to(device)
    mega_rows = sum(SIZES)
    ori_w = torch.randn(VOCAB, ORI, device=device, dtype=BF16)
    proj = (torch.randn(ORI, WIDTH, device=device) * 0.02).to(BF16)
    forms = (("128_prefill", torch.randint(0, VOCAB, (128,), device=device), torch.tensor([64, 64], device=device), 2),
             ("128_decode", torch.randint(0, VOCAB, (128, 1), device=device), None, 128),
             ("8192_prefill", torch.randint(0, VOCAB, (8192,), device=device), torch.tensor([2048] * 4, device=device), 4))
    for kind in ("dense", "nf4"):
        kw = dict(ori_vocab_size=VOCAB, ori_embed_dim=ORI, oe_embed_dim=OE, oe_vocab_sizes=torch.tensor(SIZES), oe_grams=torch.tensor(GRAMS),
                  _ori_embedding_weight=ori_w)
        if kind == "nf4":
            q, scale, mean = _nf4_table(mega_rows, OE, 64, device)
            kw.update(_mega_embedding_weight=q, _mega_embedding_scale=scale, _mega_embedding_mean=mean, _mega_embedding_group_size=64,
                      dtype=BF16)
        else:
            mega_w = torch.randn(mega_rows, OE, device=device, dtype=BF16)
            kw.update(_mega_embedding_weight=mega_w)
        layer = hip("MojoOverEncoding")(**kw)
        layer.oe_up_proj.weight = torch.nn.Parameter(proj, requires_grad=False)
        layer = layer.to(device)
        for label, ids, q_lens, batch in forms:
            name = f"oe_{label}_{kind}"
            if not _want(name):
                continue
            tokens = ids.numel()
            hist = torch.randint(0, VOCAB, (batch, 6), device=device)
            oe_ids = ngram(ids, hist, q_lens).reshape(tokens, -1)
            flat = ids.reshape(-1)
            cat = over_encoding_concat(layer, ids, hist, q_lens).reshape(tokens, WIDTH)
            mega_read = OE * 2 if kind == "dense" else OE // 2 + 2 * 4 * (OE // 64)
            nbytes = tokens * (ORI * 2 + len(SIZES) * mega_read + WIDTH * 2)

            def composition():
                if kind == "dense":
                    mega = mega_w.index_select(0, oe_ids.reshape(-1))
                else:
                    mega = _torch_nf4_rows(q, scale, mean, 64, layer.oe_mega_embedding.codebook, oe_ids.reshape(-1), BF16)
                return F.linear(torch.cat((ori_w.index_select(0, flat), mega.reshape(tokens, -1)), dim=-1), proj)

            timer = _time_graph if tokens <= 1024 else _time
            res = {"concat": _hbm(timer(lambda: over_encoding_concat(layer, ids, hist, q_lens)), nbytes),
                   "hip": _hbm(timer(lambda: layer(ids, hist, q_lens)), nbytes),
                   "gemm_alone": _hbm(timer(lambda: dense_gemm(cat, proj, None, trans_weight=False)), nbytes),
                   "torch": _hbm(timer(composition), nbytes), "tokens": tokens, "timing": "graph" if tokens <= 1024 else "eager"}
            _judge(res, "concat", nbytes, *plain)
            res["sibling"] = "gather_8192x4096"
            res["layer_allowed_us"] = res["gemm_alone"]["us"] + res["allowed_us"]
            res["layer_within_margin"] = res["hip"]["us"] <= res["layer_allowed_us"]
            res["torch_over_hip"] = res["torch"]["us"] / res["hip"]["us"]
            out[name] = res
        del layer
        torch.cuda.empty_cache()


def bench(device):
    out = {}
    plain = gather_cases(device, out)
    if plain is not None and _want("oe_"):
        over_encoding_cases(device, out, plain)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "embedding_bench.json"))
    ns = ap.parse_args()
    line = json.dumps({"embedding": bench(torch.device("cuda", 0))})
    with open(ns.out, "w") as f:
        f.write(line + "\n")
    print(line)
