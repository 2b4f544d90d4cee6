"""Exact visible-set inputs for `MojoSdpa`, in the manner of tests/visibility.py on the uniform ``[B,H,S,D]``
layout.  Everything here runs on the CPU.

* ``Q[..., 0] = 1``, ``K = 0`` and ``scale = 1``: every score is 0, so a row's weights are exactly ``1 / n`` over its ``n``
  visible keys.
* ``V`` holds one probe per (kv head, channel): channel ``c`` of kv head ``h`` is 1 at key ``probe_keys[c]`` and 0 elsewhere, so
  output channel ``c`` of a row reads ``1 / n`` if that key is visible to the row and exactly 0 if it is not.
* K and V of every batch entry are views into one larger buffer whose rows past ``Sk`` — the ``gap`` rows between two batch
  entries and behind the last — hold numeric poison: ``K[..., 0] = 256`` (a leaked key takes all the weight) and ``V = 1`` on
  every channel (so every probe, visible or not, then reads about 1).  A tail tile that reads the next batch entry, or a key
  past ``Sk``, fails every channel of the row.
"""
import torch


def probe_keys(sk, d):
    """``d`` keys of ``[0, sk)``: both sides of every multiple of 4, 16 and 64 that fits, the ends, then the rest in order."""
    edges = [0, sk - 1]
    for m in (64, 16, 4):
        for t in range(m, sk + 1, m):
            edges += [t - 1, t]
    keys = []
    for t in edges + list(range(sk)):
        if 0 <= t < sk and t not in keys:
            keys.append(t)
    return (keys * d)[:d] if len(keys) < d else keys[:d]


def build(batch, hq, hkv, sq, sk, d, dtype, gap=70):
    """(query, key, value, probe key per channel).  key / value: ``[B,Hkv,Sk,D]`` views of a ``[B, Sk + gap, Hkv, D]`` buffer."""
    q = torch.zeros(batch, hq, sq, d, dtype=dtype)
    q[..., 0] = 1
    kbuf = torch.zeros(batch, sk + gap, hkv, d, dtype=dtype)
    vbuf = torch.zeros(batch, sk + gap, hkv, d, dtype=dtype)
    kbuf[:, sk:, :, 0] = 256
    vbuf[:, sk:] = 1
    keys = probe_keys(sk, d)
    for c, t in enumerate(keys):
        vbuf[:, t, :, c] = 1
    return q, kbuf, vbuf, keys


def views(kbuf, vbuf, sk):
    return kbuf[:, :sk].transpose(1, 2), vbuf[:, :sk].transpose(1, 2)


def expected(visible, keys, dtype):
    """``visible``: bool ``[B,Hq,Sq,Sk]`` (the definition).  Returns (want ``[B,Hq,Sq,D]`` in ``dtype``, probe-visible mask)."""
    n = visible.sum(dim=-1, keepdim=True).to(torch.float32)
    share = torch.where(n > 0, 1.0 / n.clamp(min=1), torch.zeros_like(n))          # fp32(1 / n)
    seen = visible[..., torch.tensor(keys)]                                        # [B,Hq,Sq,D]: is channel c's key visible
    return torch.where(seen, share, torch.zeros_like(share)).to(dtype), seen


def compare(got, want, seen):
    """An invisible probe reads exactly 0; a visible one is within 1 ulp of storage(fp32(1 / n))."""
    assert got.shape == want.shape and got.dtype == want.dtype
    hidden = got[~seen]
    assert not bool(hidden.any()), f"{int((hidden != 0).sum())} invisible probes read non-zero (max {hidden.float().abs().max()})"
    ulps = (got[seen].view(torch.int16).to(torch.int32) - want[seen].view(torch.int16).to(torch.int32)).abs()
    assert ulps.numel() == 0 or int(ulps.max()) <= 1, f"visible probes off by up to {int(ulps.max())} ulp"
