"""The cache and block-table layouts the paged ops accept, for tests: dense CPU tensors in, views with the same values over
differently arranged storage out.  A plain helper module (no fixtures).

Every layout stays inside the documented envelope: last dimension dense, every stride a multiple of
16 bytes, 16-byte aligned base pointers, K and V with equal strides.  What a view does not cover is POISON — NaN in a 16-bit
(or fp32) cache, 127 in an int8 one — so a kernel that ignores a stride lands on it.  Hidden table columns hold the id of a
valid spare page filled with poison: no id outside the pool is ever written anywhere.

`Laid` keeps the storage next to the views: ``.to(device)`` moves the (dense) storage and re-derives the views there, which
`view.to(device)` would not (it copies a non-dense view into a dense tensor).
"""
import torch

CACHE_LAYOUTS = ("hnd", "nhd", "kv_pool", "padded")
TABLE_LAYOUTS = ("dense", "wide", "offset")
TABLE_OFFSET = 3                                   # odd: the view's base is 4-byte, not 16-byte aligned
TABLE_EXTRA = 5                                    # hidden columns of a wide table (an odd row stride for even widths)


def poison_of(dtype):
    return 127 if dtype == torch.int8 else float("nan")


def pad_elems(dtype):
    """Padding of the `padded` layout's rows: 16 bytes of 16-bit elements, 16 bytes of int8."""
    return 16 if dtype == torch.int8 else 8


class Laid:
    """Views over storage: ``views`` (tuple), ``storages`` (list of dense tensors), and the recipe between them."""

    def __init__(self, storages, recipe):
        self.storages = list(storages)
        self._recipe = recipe
        self.views = tuple(recipe(*self.storages))

    def to(self, device):
        return Laid([s.to(device) for s in self.storages], self._recipe)

    def clone(self):
        return Laid([s.clone() for s in self.storages], self._recipe)


def lay_out_kv(k, v, layout):
    """K and V ``[N, H, page, D]`` (dense) as views of that shape over ``layout``'s storage."""
    assert k.shape == v.shape and k.dtype == v.dtype and k.is_contiguous() and v.is_contiguous()
    n, h, page, d = k.shape
    if layout == "hnd":                             # dense, the baseline
        return Laid([k.clone(), v.clone()], lambda a, b: (a, b))
    if layout == "nhd":                             # token-major storage [N, page, H, D] seen through a permuted view
        return Laid([k.permute(0, 2, 1, 3).contiguous(), v.permute(0, 2, 1, 3).contiguous()],
                    lambda a, b: (a.permute(0, 2, 1, 3), b.permute(0, 2, 1, 3)))
    if layout == "kv_pool":                         # K and V are the two halves of every block of one pool
        return Laid([torch.stack([k, v], dim=1).contiguous()], lambda p: (p[:, 0], p[:, 1]))
    if layout == "padded":                          # a block in front, a token row and `pad` elements behind each row
        pad = pad_elems(k.dtype)
        stores = []
        for t in (k, v):
            s = torch.full((n + 1, h, page + 1, d + pad), poison_of(t.dtype), dtype=t.dtype)
            s[1:, :, :page, :d] = t
            stores.append(s)
        return Laid(stores, lambda a, b: (a[1:, :, :page, :d], b[1:, :, :page, :d]))
    raise ValueError(layout)


def lay_out_mla(ckv, kpe, layout):
    """The MLA caches ``[N, 1, page, r]`` / ``[N, 1, page, rope]``: dense, or `fused_row` — one storage whose rows hold
    ``c_kv | k_pe``."""
    assert ckv.shape[:3] == kpe.shape[:3] and ckv.shape[1] == 1
    if layout == "dense":
        return Laid([ckv.clone(), kpe.clone()], lambda a, b: (a, b))
    if layout == "fused_row":
        r = ckv.shape[3]
        return Laid([torch.cat([ckv, kpe], dim=3).contiguous()], lambda s: (s[..., :r], s[..., r:]))
    raise ValueError(layout)


def spare_pages(n_blocks, table):
    """Ids of the pool's pages that ``table`` does not name, ascending."""
    return sorted(set(range(n_blocks)) - set(table[table >= 0].tolist()))


def poison_page(caches, page_id):
    """Fill page ``page_id`` of every cache with poison (in place); returns ``page_id``."""
    for c in caches:
        c[page_id] = poison_of(c.dtype)
    return page_id


def lay_out_table(table, layout, hidden_id):
    """The block table ``[B, w]`` as a column slice of a wider table whose hidden columns all hold ``hidden_id`` (a valid
    page of the pool, poisoned by the caller): `wide` = ``wide[:, :w]`` (row stride only), `offset` =
    ``wide[:, c:c + w]`` with odd ``c`` (row stride and a base that is only 4-byte aligned)."""
    assert table.dtype == torch.int32 and table.dim() == 2
    b, w = table.shape
    if layout == "dense":
        return Laid([table.clone()], lambda t: (t,))
    c = {"wide": 0, "offset": TABLE_OFFSET}[layout]
    wide = torch.full((b, w + c + TABLE_EXTRA), int(hidden_id), dtype=torch.int32)
    wide[:, c:c + w] = table
    return Laid([wide], lambda t: (t[:, c:c + w],))


def in_envelope(t):
    """Last dimension dense, every other stride a multiple of 16 bytes, base pointer 16-byte aligned."""
    es = t.element_size()
    return t.stride(-1) == 1 and all((s * es) % 16 == 0 for s in t.stride()[:-1]) and t.data_ptr() % 16 == 0
