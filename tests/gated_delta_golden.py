"""References of the gated-delta-rule ops (`LINEAR_ATTN_OPS`): the token loop in fp64, the chunk algebra at the kernel's precision,
and the case builder of tests/test_hip_gated_delta.py.  Written from the formulas (the textbook form with U and W), not from the kernel."""
import functools

import torch

C = 64


def _normed(x, on):
    x = x.double()
    return x * torch.rsqrt((x * x).sum(-1, keepdim=True) + 1e-6) if on else x


def model64(q, k, v, g, beta, state=None, scale=None, norm=True):
    """One sequence, ``q`` / ``k`` [T, Hk, Dk], ``v`` [T, Hv, Dv], ``g`` / ``beta`` [T, Hv], ``state`` [Hv, Dk, Dv] or None: the
    recurrence in fp64 on the stored inputs.  Returns ``(out [T, Hv, Dv], final state, scale |S|^T |q^| per token, sum_t |k^| (x) |d|, sum_t |S|)``
    (the last three are the magnitudes the update op's fp32 bound runs over)."""
    group = v.shape[1] // q.shape[1]
    q, k = _normed(q, norm).repeat_interleave(group, 1), _normed(k, norm).repeat_interleave(group, 1)
    v, g, beta = v.double(), g.double(), beta.double()
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    s = torch.zeros(v.shape[1], q.shape[2], v.shape[2], dtype=torch.float64) if state is None else state.double().clone()
    out, mag_o, mag_kd, mag_s = torch.empty_like(v), torch.empty_like(v), torch.zeros_like(s), torch.zeros_like(s)
    for t in range(q.shape[0]):
        s = s * torch.exp(g[t])[:, None, None]
        d = beta[t][:, None] * (v[t] - torch.einsum("hkv,hk->hv", s, k[t]))
        s = s + k[t][:, :, None] * d[:, None, :]
        out[t] = scale * torch.einsum("hkv,hk->hv", s, q[t])
        mag_o[t] = scale * torch.einsum("hkv,hk->hv", s.abs(), q[t].abs())
        mag_kd, mag_s = mag_kd + k[t].abs()[:, :, None] * d.abs()[:, None, :], mag_s + s.abs()
    return out, s, mag_o, mag_kd, mag_s


def chunk_bf16_yardstick(q, k, v, g, beta, state=None, scale=None, norm=True, operand=torch.bfloat16):
    """The same sequence through the chunk algebra (C = 64) in fp32 with every matrix operand rounded to ``operand``."""
    rnd = lambda x: x.to(operand).float()                                        # noqa: E731
    mm = lambda a, b: rnd(a) @ rnd(b)                                            # noqa: E731
    tokens, group = q.shape[0], v.shape[1] // q.shape[1]
    qn = _normed(q, norm).float().repeat_interleave(group, 1)
    kn = _normed(k, norm).float().repeat_interleave(group, 1)
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    s = torch.zeros(v.shape[1], q.shape[2], v.shape[2]) if state is None else state.float().clone()
    out = torch.empty(v.shape, dtype=torch.float32)
    low, eye = torch.tril(torch.ones(C, C, dtype=torch.bool)), torch.eye(C)
    for h in range(v.shape[1]):
        for c0 in range(0, tokens, C):
            n = min(C, tokens - c0)
            pad = lambda x: torch.cat([x[c0:c0 + n, h].float(), torch.zeros(C - n, *x.shape[2:])])   # noqa: E731
            kc, qc, vc, gc, bc = pad(kn), pad(qn), pad(v), pad(g), pad(beta)
            big_g = gc.cumsum(0)
            gamma = torch.where(low, torch.exp(torch.where(low, big_g[:, None] - big_g[None, :], 0.0)), 0.0)
            a = torch.where(low & ~eye.bool(), bc[:, None] * mm(kc, kc.T) * gamma, 0.0)
            tm = torch.linalg.solve_triangular(eye + a, eye, upper=False)
            w, u = mm(tm, (bc * torch.exp(big_g))[:, None] * kc), mm(tm, bc[:, None] * vc)
            vn = u - mm(w, s[h])
            o = scale * (mm(torch.exp(big_g)[:, None] * qc, s[h]) + mm(mm(qc, kc.T) * gamma, vn))
            s[h] = torch.exp(big_g[-1]) * s[h] + mm((torch.exp(big_g[-1] - big_g)[:, None] * kc).T, vn)
            out[c0:c0 + n, h] = o[:n]
    return out, s


@functools.lru_cache(maxsize=None)
def build(tokens, dk, dv, hk, hv, norm=True, init=True, dtype=torch.bfloat16, edge=False, seed=0):
    """One sequence of seeded inputs with its fp64 model, cached and never modified.  Without the norm ``k`` is scaled by
    ``Dk ** -0.5`` so the recurrence stays contractive.  ``edge``: g = 0 for the first third, g = -8 per token for the second
    (the decay underflows inside a chunk), beta 0 on every third token and 1 on the next."""
    gen = torch.Generator().manual_seed(seed * 1000 + tokens + dk + 3 * dv + 7 * hk + 11 * hv)
    r = lambda *s: torch.randn(*s, generator=gen)                                 # noqa: E731
    q, k, v = r(tokens, hk, dk), r(tokens, hk, dk), r(tokens, hv, dv)
    if not norm:
        k = k * dk ** -0.5
    g = -torch.nn.functional.softplus(r(tokens, hv)) * 0.3
    beta = torch.sigmoid(r(tokens, hv))
    if edge:
        g[:tokens // 3] = 0.0
        g[tokens // 3:2 * tokens // 3] = -8.0
        beta[0::3], beta[1::3] = 0.0, 1.0
    c = dict(q=q.to(dtype), k=k.to(dtype), v=v.to(dtype), g=g, beta=beta, norm=norm,
             state=r(hv, dk, dv) * 0.5 if init else None)
    c["out64"], c["state64"], c["mag_o"], c["mag_kd"], c["mag_s"] = model64(c["q"], c["k"], c["v"], g, beta, c["state"], norm=norm)
    return c
