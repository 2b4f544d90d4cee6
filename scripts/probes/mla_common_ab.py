"""A/B of the MLA latent attention between two libraries (MOJO_HIP_LIB selects the one a process loads):

    MOJO_HIP_LIB=<parent>/libmojo_hip.so python3 scripts/probes/mla_common_ab.py bits  a.pt      # every case's output
    python3 scripts/probes/mla_common_ab.py bits b.pt                                            # this tree's library
    python3 scripts/probes/mla_common_ab.py compare a.pt b.pt [out.json]                         # torch.equal, case by case
    [MOJO_HIP_LIB=...] python3 scripts/probes/mla_common_ab.py speed out.json                    # the timed cases, medians

One library per process (a fresh child each): the library latches its switches and its per-device launch attributes.
`bits`: decode, B 4, lengths {0, 1, 65, 1000} over a 1024-token table — heads 16 / 72 / 128 (one head block, a partial
second, two), (r, rope) = (512, 64) and (64, 32), page 16 (`ps`), page 8 (`oct`) and MOJO_HIP_MLA_KERNEL=oct at page 16,
MOJO_HIP_MLA_SPLITS unset / 1 / 5, sink on / off, bf16 / fp16, and a table with a negative id in mid-row; absorbed prefill
(MOJO_HIP_MLA_PREFILL=absorbed) of q_lens [3, 17] over cached [0, 40], also with cu_q[0] > 0 and trailing padding rows.
`speed`: the decode headline of benchmarks/extras.py, the absorbed route of its two prefill cases, an eager decode call at
B 1 / ctx 256 (host path and launch attributes dominate there)."""
import itertools
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
DIMS = {512: dict(nope=128, rope=64, vd=128), 64: dict(nope=64, rope=32, vd=64)}
LENS, TABLE_TOKENS = (0, 1, 65, 1000), 1024
SWITCHES = ("MOJO_HIP_MLA_KERNEL", "MOJO_HIP_MLA_SPLITS", "MOJO_HIP_MLA_PREFILL")


def set_env(**values):
    from mojo_opset_amd import switches

    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update({k: v for k, v in values.items() if v is not None})
    switches.reload()


def make_op(name, heads, r, sink, dtype, seed):
    import mojo_opset_amd as mo

    d = DIMS[r]
    g = torch.Generator().manual_seed(seed)
    op = getattr(mo, name).get_backend_impl("hip", strict=True)(heads, d["nope"], d["rope"], d["vd"], r, use_attn_sink=sink)
    op = op.to(dtype).to(DEV)
    with torch.no_grad():
        op.kv_b_proj.copy_((torch.randn(heads * (d["nope"] + d["vd"]), r, generator=g) * 0.1).to(dtype))
        if sink:
            op.attn_sink.copy_(torch.randn(heads, generator=g))
    return op


def make_cache(kv_lens, r, page, width, dtype, seed):
    """Caches of random pages and a table of `width` columns: a sequence's pages, then valid ids of pages nobody owns."""
    g = torch.Generator().manual_seed(seed)
    total = len(kv_lens) * width + 3
    ckv = torch.randn(total, 1, page, r, generator=g).to(dtype)
    kpe = torch.randn(total, 1, page, DIMS[r]["rope"], generator=g).to(dtype)
    table = torch.randperm(total, generator=g, dtype=torch.int32)[: len(kv_lens) * width].view(len(kv_lens), width)
    return ckv.to(DEV), kpe.to(DEV), table


def cu(lens, first=0):
    return torch.tensor([first] + [first + x for x in itertools.accumulate(lens)], dtype=torch.int32, device=DEV)


def bits_cases():
    """(name, environment, thunk) — the thunk builds its inputs from fixed seeds and returns the op's output."""
    for heads, r, dtype, sink in itertools.product((16, 72, 128), (512, 64), (torch.bfloat16, torch.float16), (False, True)):
        kernels = (("p16", 16, None), ("p8", 8, None)) + ((("p16oct", 16, "oct"),) if r == 512 else ())
        for (ktag, page, kernel), splits, hole in itertools.product(kernels, (None, "1", "5"), (False, True)):
            if hole and (sink or dtype is torch.float16):
                continue

            def decode(heads=heads, r=r, dtype=dtype, sink=sink, page=page, hole=hole):
                op = make_op("MojoPagedDecodeMLA", heads, r, sink, dtype, 1)
                ckv, kpe, table = make_cache(LENS, r, page, TABLE_TOKENS // page, dtype, 2)
                if hole:
                    table[3, (TABLE_TOKENS // page) // 3] = -1           # the 1000-key row loses its tail in mid-row
                q = torch.randn(len(LENS), heads, DIMS[r]["nope"] + DIMS[r]["rope"], generator=torch.Generator().manual_seed(3)).to(dtype)
                return op(q.to(DEV), ckv, kpe, torch.tensor(LENS, dtype=torch.int32, device=DEV), table.to(DEV))

            name = f"decode-h{heads}-r{r}-{str(dtype)[6:]}-{ktag}-splits{splits or 'default'}{'-sink' if sink else ''}{'-hole' if hole else ''}"
            yield name, dict(MOJO_HIP_MLA_KERNEL=kernel, MOJO_HIP_MLA_SPLITS=splits), decode
        for splits, first in itertools.product((None, "1", "5"), (0, 2)):
            q_lens, cached, page = (3, 17), (0, 40), 16

            def prefill(heads=heads, r=r, dtype=dtype, sink=sink, first=first):
                op = make_op("MojoPagedPrefillMLA", heads, r, sink, dtype, 4)
                kv = [a + b for a, b in zip(q_lens, cached)]
                ckv, kpe, table = make_cache(kv, r, page, 8, dtype, 5)
                rows = first + sum(q_lens) + (3 if first else 0)             # cu_q[0] > 0: padding in front and behind
                q = torch.randn(rows, heads, DIMS[r]["nope"] + DIMS[r]["rope"], generator=torch.Generator().manual_seed(6)).to(dtype)
                return op(q.to(DEV), ckv, kpe, cu(q_lens, first), table.to(DEV), cu_total_seq_lens=cu(kv))

            name = f"prefill-h{heads}-r{r}-{str(dtype)[6:]}-splits{splits or 'default'}{'-sink' if sink else ''}{'-padded' if first else ''}"
            yield name, dict(MOJO_HIP_MLA_PREFILL="absorbed", MOJO_HIP_MLA_SPLITS=splits), prefill


def run_bits(path):
    from mojo_opset_amd.backends.hip import lib as L

    out, launches = {}, {}
    for name, env, thunk in bits_cases():
        set_env(**env)
        L.launch_history(clear=True)
        out[name] = thunk().cpu()
        launches[name] = L.launch_history()
    torch.cuda.synchronize()
    torch.save({"library": L.load().mojo_hip_version().decode(), "out": out, "launches": launches}, path)
    print(len(out), "cases ->", path, "|", L.load().mojo_hip_version().decode())


def run_compare(path_a, path_b, path_json=None):
    a, b = torch.load(path_a), torch.load(path_b)
    cases = {}
    for name in a["out"]:
        mla = [x for x in a["launches"][name].split("|") if x.startswith("mla")]
        cases[name] = {"equal": bool(torch.equal(a["out"][name], b["out"][name])), "same_launches": a["launches"][name] == b["launches"][name],
                       "launch": "|".join(mla), "finite": bool(torch.isfinite(a["out"][name].float()).all())}
    res = {"a": a["library"], "b": b["library"], "cases": len(cases), "all_equal": all(c["equal"] for c in cases.values()),
           "all_same_launches": all(c["same_launches"] for c in cases.values()), "by_case": cases}
    if set(a["out"]) != set(b["out"]):
        res["all_equal"] = False
    print(json.dumps({k: v for k, v in res.items() if k != "by_case"}))
    for name, c in cases.items():
        if not (c["equal"] and c["same_launches"]):
            print("DIFFERS", name, c)
    if path_json:
        with open(path_json, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if res["all_equal"] and res["all_same_launches"] else 1


def run_speed(path):
    from benchmarks import extras
    from mojo_opset_amd.backends.hip import lib as L

    timed = []
    inner = extras._time

    def recording(*args, **kwargs):
        t = inner(*args, **kwargs)
        timed.append({"us": t * 1e6, **extras._stats(t)})
        return t

    extras._time = recording
    os.environ["MOJO_BENCH_ONLY"] = "4x512"                        # (no case of bench_mla_decode but the headline matches)
    dev = torch.device(DEV)
    res = {}
    extras.bench_mla_decode(dev)
    res["mla_decode_B64_H128_ctx4096_page16"] = timed[0]
    del timed[:]
    extras.bench_mla_prefill(dev)
    res["mla_prefill_4x512_nocache:absorbed_route"] = timed[1]
    res["mla_prefill_4x512_cached2048:absorbed_route"] = timed[3]
    extras._time = inner
    set_env()
    op = make_op("MojoPagedDecodeMLA", 128, 512, False, torch.bfloat16, 1)
    ckv, kpe, table = make_cache((256,), 512, 16, 16, torch.bfloat16, 2)
    q = torch.randn(1, 128, 192, device=DEV, dtype=torch.bfloat16)
    lens, table = torch.tensor([256], dtype=torch.int32, device=DEV), table.to(DEV)
    t = inner(lambda: op(q, ckv, kpe, lens, table), iters=200, warmup=5)
    res["mla_decode_eager_B1_ctx256"] = {"us": t * 1e6, **extras._stats(t)}
    res["library"] = L.load().mojo_hip_version().decode()
    print(json.dumps(res))
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "bits":
        run_bits(sys.argv[2])
    elif mode == "compare":
        sys.exit(run_compare(*sys.argv[2:5]))
    else:
        run_speed(sys.argv[2])
