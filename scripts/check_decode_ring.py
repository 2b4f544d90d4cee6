"""Check that the hot loop of every `decode_mfma_kernel` instance really keeps K/V tiles in flight (compiled gfx950 assembly).

The kernel's ring holds three tiles in registers: one is processed while the loads of the next two are outstanding.  Vector
memory loads return in order and `s_waitcnt vmcnt(N)` waits until at most N of them are outstanding, so the depth the ring
really reaches can be read off the loop's waits.  Two things took it to a single buffer without changing one result:

  * the page id of every tile came from a `global_load_dword` followed by `s_waitcnt vmcnt(0)` and `v_readfirstlane_b32`:
    the wait for the id retired every K/V load issued before it, and only then was the next tile requested;
  * every tile load of the loop was conditional, so the compiler waited as if the tile being processed could be the last
    one issued: `vmcnt(7) ... vmcnt(0)` right after requesting the next tile.

Rules enforced here, in the innermost loop that holds the most `v_mfma` instructions of each such kernel:

  * no `s_waitcnt` leaves fewer vector loads outstanding than one loop step issues (8: a step moves 8 KiB, 16 bytes a lane);
  * no single-dword global load feeds a `v_readfirstlane`;

in the blocks of the loop around it that belong to that loop alone — where the ring hands its page-id window over between two
rounds (a copy placed behind the refill waited `vmcnt(0)` there: both tiles in flight drained once per window) —

  * no `s_waitcnt` leaves fewer than 8 vector loads outstanding either;

and, from the compiler's resource remarks (`-Rpass-analysis=kernel-resource-usage`, printed to stderr), no scratch.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -Rpass-analysis=kernel-resource-usage \
        -o k.s paged_decode_gqa.hip 2> k.remarks && python scripts/check_decode_ring.py k.s k.remarks

The checker reads only labels, branches, waits, loads, lane reads and MFMAs.  tests/test_isa_decode_ring.py runs it.
"""
import re
import sys

KERNEL = "decode_mfma_kernel"
STEP_LOADS = 8

_LABEL = re.compile(r"^([.\w$]+):")
_BRANCH = re.compile(r"^\s*(s_branch|s_cbranch_\w+)\s+([.\w$]+)")
_WAIT_VM = re.compile(r"^\s*s_waitcnt\b.*\bvmcnt\((\d+)\)")
_VLOAD = re.compile(r"^\s*(global_load_\w+|buffer_load_\w+|flat_load_\w+|scratch_load_\w+)\s+(v\[\d+:\d+\]|v\d+)\s*,")
_DWORD = re.compile(r"^\s*global_load_dword\s+v(\d+)\s*,")
_RFL = re.compile(r"^\s*v_readfirstlane_b32\s+s\d+\s*,\s*v(\d+)\b")
_DEF = re.compile(r"^\s*[vd]\w+\s+(v\[(\d+):(\d+)\]|v(\d+))\b")


def functions(lines):
    """[(name, [line, ...])] of the kernels in an assembly listing (from a `name:` label to .Lfunc_end)."""
    out, cur, name = [], None, None
    for ln in lines:
        m = _LABEL.match(ln)
        if m and not m.group(1).startswith(".L") and cur is None and not ln.startswith("\t"):
            name, cur = m.group(1), []
            continue
        if cur is not None:
            cur.append(ln.split(";")[0].rstrip())
            if ln.startswith(".Lfunc_end"):
                out.append((name, cur))
                cur = None
    return out


def _loops(body):
    """[(first, last)] of every span from a label to a branch back to it."""
    labels = {}
    for i, ln in enumerate(body):
        m = _LABEL.match(ln)
        if m:
            labels[m.group(1)] = i
    spans = []
    for i, ln in enumerate(body):
        b = _BRANCH.match(ln)
        if b and b.group(2) in labels and labels[b.group(2)] < i:
            spans.append((labels[b.group(2)], i))
    return spans


def hot_loop(body):
    """(first, last) line of the innermost loop with the most v_mfma instructions, or None.  A loop is the span from a label
    to a branch back to it; innermost: no other such span lies inside it."""
    spans = _loops(body)
    inner = [s for s in spans if not any(o != s and s[0] <= o[0] and o[1] <= s[1] for o in spans)]
    best, best_n = None, 0
    for lo, hi in inner:
        n = sum(1 for ln in body[lo: hi + 1] if ln.lstrip().startswith("v_mfma"))
        if n > best_n:
            best, best_n = (lo, hi), n
    return best


def enclosing_blocks(body, span):
    """Line numbers of the loops around `span` outside `span` itself: where the ring changes its id window between two
    rounds.  These are the lines that lie on a cycle through the hot loop's first line — found on the control-flow graph,
    not by position: the compiler lays blocks of other loops (and of no loop) between them.  Empty when nothing encloses it."""
    labels = {}
    for i, ln in enumerate(body):
        m = _LABEL.match(ln)
        if m:
            labels[m.group(1)] = i
    n = len(body)
    succ = [[] for _ in range(n)]
    for i, ln in enumerate(body):
        b = _BRANCH.match(ln)
        if b and b.group(2) in labels:
            succ[i].append(labels[b.group(2)])
        if i + 1 < n and not (b and b.group(1) == "s_branch") and not ln.lstrip().startswith("s_endpgm"):
            succ[i].append(i + 1)
    pred = [[] for _ in range(n)]
    for i, out in enumerate(succ):
        for j in out:
            pred[j].append(i)

    def reach(start, edges):
        seen, work = {start}, [start]
        while work:
            for j in edges[work.pop()]:
                if j not in seen:
                    seen.add(j)
                    work.append(j)
        return seen

    cycle = reach(span[0], succ) & reach(span[0], pred)
    return sorted(i for i in cycle if not span[0] <= i <= span[1])


def _defines(ln, reg):
    m = _DEF.match(ln)
    if not m:
        return False
    if m.group(4) is not None:
        return int(m.group(4)) == reg
    return int(m.group(2)) <= reg <= int(m.group(3))


def check_function(name, body):
    """(stats, violations) of one kernel: stats = MFMAs, vector loads and the smallest vmcnt of its hot loop."""
    span = hot_loop(body)
    if span is None:
        return ({"mfma": 0, "loads": 0, "min_vmcnt": None, "outer_lines": 0, "outer_loads": 0, "outer_min_vmcnt": None},
                [f"{name}: no loop with v_mfma instructions"])
    loop = body[span[0]: span[1] + 1]
    out = []
    waits = []
    for i, ln in enumerate(loop):
        w = _WAIT_VM.match(ln)
        if w:
            waits.append(int(w.group(1)))
            if int(w.group(1)) < STEP_LOADS:
                out.append(f"{name}: loop +{i}: `{ln.strip()}` leaves fewer than {STEP_LOADS} vector loads outstanding")
    own = enclosing_blocks(body, span)
    outer_waits = []
    for i in own:                                           # the window hand-over: a drain here empties the ring once per window
        w = _WAIT_VM.match(body[i])
        if w:
            outer_waits.append(int(w.group(1)))
            if int(w.group(1)) < STEP_LOADS:
                out.append(f"{name}: enclosing loop +{i - own[0]}: `{body[i].strip()}` leaves fewer than {STEP_LOADS} vector loads outstanding")
    n = len(loop)
    for i, ln in enumerate(loop):
        d = _DWORD.match(ln)
        if not d:
            continue
        reg = int(d.group(1))
        for k in range(1, n):                               # once round the loop, until the register is written again
            nxt = loop[(i + k) % n]
            r = _RFL.match(nxt)
            if r and int(r.group(1)) == reg:
                out.append(f"{name}: loop +{i}: `{ln.strip()}` feeds `{nxt.strip()}`: a memory round trip per tile")
                break
            if _defines(nxt, reg):
                break
    stats = {"mfma": sum(1 for ln in loop if ln.lstrip().startswith("v_mfma")),
             "loads": sum(1 for ln in loop if _VLOAD.match(ln)),
             "min_vmcnt": min(waits) if waits else None,
             "outer_lines": len(own), "outer_loads": sum(1 for i in own if _VLOAD.match(body[i])),
             "outer_min_vmcnt": min(outer_waits) if outer_waits else None}
    return stats, out


def check_listing(lines):
    """{kernel: stats}, [violation, ...] over every decode_mfma_kernel of a listing."""
    stats, report = {}, []
    for name, body in functions(lines):
        if KERNEL not in name:
            continue
        stats[name], bad = check_function(name, body)
        report += bad
    return stats, report


def resources(remarks):
    """{kernel: {"vgprs", "agprs", "scratch", "occupancy", "vgpr_spill"}} from the text of the compiler's resource remarks."""
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
            "VGPRs Spill": "vgpr_spill"}
    out, cur = {}, None
    for ln in remarks.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+)\s+\[-Rpass-analysis", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {}) if KERNEL in m.group(2) else None
        elif cur is not None and m.group(1).strip() in keys:
            cur[keys[m.group(1).strip()]] = int(m.group(2))
    return out


def check_resources(remarks):
    res = resources(remarks)
    return res, [f"{k}: {v.get('scratch')} bytes of scratch per lane ({v.get('vgpr_spill')} spilled VGPRs)"
                 for k, v in res.items() if v.get("scratch", 1) != 0]


if __name__ == "__main__":
    with open(sys.argv[1]) as f:
        stats, report = check_listing(f.readlines())
    res = {}
    if len(sys.argv) > 2:
        with open(sys.argv[2]) as f:
            res, bad = check_resources(f.read())
        report += bad
    for k, s in stats.items():
        r = res.get(k, {})
        print(f"{k}: loop of {s['mfma']} MFMAs, {s['loads']} vector loads, smallest vmcnt {s['min_vmcnt']}; enclosing loop: "
              f"{s['outer_lines']} lines, {s['outer_loads']} loads, smallest vmcnt {s['outer_min_vmcnt']}; "
              f"VGPRs {r.get('vgprs')} AGPRs {r.get('agprs')} scratch {r.get('scratch')} occupancy {r.get('occupancy')}")
    for r in report:
        print("  " + r)
    sys.exit(1 if report else 0)
