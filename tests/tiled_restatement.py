"""Tiled inference (include/dptx.h "Tiled inference", omnidata_amd/tiled.py), restated literally in torch: every tile decoded or
clamped at its own resolution and F.interpolate'd into its window, the feathered weight planes, the weighted sums in grid order,
and for depth the four sums of every tile against the anchor over its window with the 2 x 2 solve (tta_depth_restatement.py's
arithmetic).  dtype torch.float32 is the composition a user would write; torch.float64 is the reference the tests measure
against.  Also the synthetic cases the host tests, the host build and the GPU tests share."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

DEGENERATE = 1e-10
Grid = namedtuple("Grid", "ys xs ch cw ry rx")      # starts per axis (tuples: a Grid is hashable), the window, the ramps


def starts(L, c, r):
    """The planner's starts along an axis (omnidata_amd/tiled.py), restated."""
    if c == L:
        return [0]
    n = -(-(L - r) // (c - r))
    return [(i * (L - c) + (n - 1) // 2) // (n - 1) for i in range(n)]


def axis_weight(c, r, s, L, dtype):
    """[c] weights of a window of c pixels at start s of an axis of length L with ramp r."""
    t = torch.arange(c, dtype=dtype)
    one = torch.ones(c, dtype=dtype)
    left = one if (s == 0 or r == 0) else torch.minimum(one, (t + 0.5) / r)
    right = one if (s + c == L or r == 0) else torch.minimum(one, ((c - 1 - t) + 0.5) / r)
    return left * right


def tile_weight(grid, iy, ix, size, dtype):
    H, W = size
    return axis_weight(grid.ch, grid.ry, grid.ys[iy], H, dtype)[:, None] * axis_weight(grid.cw, grid.rx, grid.xs[ix], W, dtype)[None, :]


def _resize(v, ch, cw):
    return F.interpolate(v[None], (ch, cw), mode="bilinear", align_corners=False)[0]


def blend_normals_restatement(maps, grid, size, dtype=torch.float32, normalize_views=True):
    """maps: the tiles' [3,h,w] fp32 maps in grid order -> [3,H,W] in `dtype`: the encoded, clamped blend (the "f32" output)."""
    H, W = size
    acc = torch.zeros(3, H, W, dtype=dtype)
    for k, m in enumerate(maps):
        iy, ix = divmod(k, len(grid.xs))
        n = 2 * m.to(dtype) - 1
        if normalize_views:
            n = F.normalize(n, dim=0, eps=1e-12)
        v = _resize(n, grid.ch, grid.cw)
        y0, x0 = grid.ys[iy], grid.xs[ix]
        acc[:, y0:y0 + grid.ch, x0:x0 + grid.cw] += tile_weight(grid, iy, ix, size, dtype) * v
    return ((F.normalize(acc, dim=0, eps=1e-12) + 1) / 2).clamp(0, 1)


def to_u8(encoded):
    """ToPILImage's mul(255).byte(): truncation.  [3,H,W] -> [H,W,3] uint8"""
    return (encoded * 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def blend_depth_restatement(maps, grid, size, anchor=None, dtype=torch.float32, align=True):
    """maps: the tiles' [h,w] fp32 maps in grid order; anchor: the whole image's [ah,aw] map (needed with align) ->
    (out [H,W] in `dtype`: 1 - blended depth, coeffs [tiles, 2] in `dtype`; (1, 0) rows with align=False)."""
    H, W = size
    coeffs = torch.zeros(len(maps), 2, dtype=dtype)
    coeffs[:, 0] = 1
    a_full = _resize(anchor.to(dtype).clamp(0, 1)[None], H, W)[0] if align else None
    acc, wsum = torch.zeros(H, W, dtype=dtype), torch.zeros(H, W, dtype=dtype)
    for k, m in enumerate(maps):
        iy, ix = divmod(k, len(grid.xs))
        y0, x0 = grid.ys[iy], grid.xs[ix]
        r = _resize(m.to(dtype).clamp(0, 1)[None], grid.ch, grid.cw)[0]
        if align:
            a = a_full[y0:y0 + grid.ch, x0:x0 + grid.cw]
            n = torch.tensor(float(grid.ch * grid.cw), dtype=dtype)
            sr, srr, sa, sra = r.sum(), (r * r).sum(), a.sum(), (r * a).sum()
            det = n * srr - sr * sr
            if bool(det > DEGENERATE * n * srr):
                coeffs[k, 0] = (n * sra - sr * sa) / det
                coeffs[k, 1] = (srr * sa - sr * sra) / det
            else:
                coeffs[k, 1] = (sa - sr) / n
        w = tile_weight(grid, iy, ix, size, dtype)
        acc[y0:y0 + grid.ch, x0:x0 + grid.cw] += w * (coeffs[k, 0] * r + coeffs[k, 1])
        wsum[y0:y0 + grid.ch, x0:x0 + grid.cw] += w
    return 1 - (acc / wsum).clamp(0, 1), coeffs


# ------------------------------------------------------------------------------------------------ the cases the tests share
SIZE = (97, 150)                                                        # (H, W): the 150 x 97 image
GRID = Grid(tuple(starts(97, 48, 12)), tuple(starts(150, 64, 16)), 48, 64, 12, 16)    # 64 x 48 windows, ramps 16 and 12: 3 x 3 tiles
NET = (32, 32)                                                          # a real resize on both axes
ANCHOR_NET = (40, 56)
assert GRID.ys == (0, 25, 49) and GRID.xs == (0, 43, 86)


def truth(size, ys=None, xs=None):
    """0.45 + 0.15 sin(x / 17) cos(y / 11) at rows ys and columns xs (pixel indices; the image's own by default), fp64."""
    H, W = size
    ys = torch.arange(H, dtype=torch.float64) if ys is None else ys
    xs = torch.arange(W, dtype=torch.float64) if xs is None else xs
    Y, X = torch.meshgrid(ys, xs, indexing="ij")
    return 0.45 + 0.15 * torch.sin(X / 17.0) * torch.cos(Y / 11.0)


def planted(k):
    """(s, t) of tile k: s in [0.8, 1.25], t in [-0.1, 0.1], seeded."""
    g = torch.Generator().manual_seed(4000 + k)
    a, b = (float(v) for v in torch.rand(2, generator=g, dtype=torch.float64))
    return 0.8 + 0.45 * a, -0.1 + 0.2 * b


def _sample_rows(start, c, n):
    """the image coordinates that the n pixels of a map of a window [start, start + c) look at"""
    return start - 0.5 + (torch.arange(n, dtype=torch.float64) + 0.5) * c / n


@functools.lru_cache(maxsize=None)
def depth_case(grid=GRID, size=SIZE, net=NET, anchor_net=ANCHOR_NET, noise=0.01):
    """-> (tile maps, anchor map): the truth sampled at every tile's network resolution, seen through the tile's planted map
    ((truth - t) / s, so that s * map + t is the truth) plus a little noise; the anchor sees the truth itself."""
    g = torch.Generator().manual_seed(77)
    maps = []
    for k in range(len(grid.ys) * len(grid.xs)):
        iy, ix = divmod(k, len(grid.xs))
        s, t = planted(k)
        m = (truth(size, _sample_rows(grid.ys[iy], grid.ch, net[0]), _sample_rows(grid.xs[ix], grid.cw, net[1])) - t) / s
        maps.append((m + noise * torch.randn(net, generator=g, dtype=torch.float64)).float())
    H, W = size
    anchor = truth(size, _sample_rows(0, H, anchor_net[0]), _sample_rows(0, W, anchor_net[1]))
    return tuple(maps), (anchor + noise * torch.randn(anchor_net, generator=g, dtype=torch.float64)).float()


@functools.lru_cache(maxsize=None)
def depth_reference(align=True):
    """-> (fp64 out, fp64 coeffs, e_ref, e_ref_c) of depth_case(): e_ref / e_ref_c = the fp32 restatement's own distance from
    the fp64 one, output and coefficients."""
    maps, anchor = depth_case()
    o64, c64 = blend_depth_restatement(maps, GRID, SIZE, anchor, torch.float64, align)
    o32, c32 = blend_depth_restatement(maps, GRID, SIZE, anchor, torch.float32, align)
    return o64, c64, float((o32.double() - o64).abs().max()), float((c32.double() - c64).abs().max())


@functools.lru_cache(maxsize=None)
def normal_case(grid=GRID, net=NET, seed=5):
    """-> the tiles' [3,h,w] maps: smooth random normals with a dominant z, encoded to [0, 1], not unit length."""
    g = torch.Generator().manual_seed(seed)
    maps = []
    for _ in range(len(grid.ys) * len(grid.xs)):
        low = torch.randn(1, 3, 5, 5, generator=g)
        n = F.interpolate(low, net, mode="bicubic", align_corners=True)[0] * 0.5
        n[2] += 1.0
        n = n * (0.7 + 0.6 * torch.rand(1, *net, generator=g))
        maps.append(((n + 1) / 2).clamp(0, 1).float())
    return tuple(maps)


@functools.lru_cache(maxsize=None)
def normal_reference(normalize_views=True):
    """-> (fp64 encoded blend [3,H,W], the fp32 restatement's one, e_ref) of normal_case()."""
    maps = normal_case()
    o64 = blend_normals_restatement(maps, GRID, SIZE, torch.float64, normalize_views)
    o32 = blend_normals_restatement(maps, GRID, SIZE, torch.float32, normalize_views)
    return o64, o32, float((o32.double() - o64).abs().max())


def u8_differences(a, b):
    """-> (largest difference in levels, fraction of bytes that differ) of two uint8 tensors"""
    d = (a.to(torch.int16) - b.to(torch.int16)).abs()
    return int(d.max()), float((d > 0).double().mean())


def crops_of(full, grid):
    """every tile the exact crop of one map `full` ([C,H,W] or [H,W]): h == ch, w == cw"""
    return tuple(full[..., y0:y0 + grid.ch, x0:x0 + grid.cw].contiguous() for y0 in grid.ys for x0 in grid.xs)


@functools.lru_cache(maxsize=None)
def seam_case():
    """-> (one random depth map [H,W] in [0, 1], one random field of unit normals encoded [3,H,W]) for the seam condition"""
    g = torch.Generator().manual_seed(11)
    depth = torch.rand(SIZE, generator=g)
    n = F.normalize(torch.randn(3, *SIZE, generator=g, dtype=torch.float64), dim=0)
    return depth, ((n + 1) / 2).float()


@functools.lru_cache(maxsize=None)
def planted_case():
    """The planted case at 1:1: the tiles see (truth - t) / s of their windows exactly, the anchor is the truth.
    -> (tile maps, anchor, truth fp64)"""
    tr = truth(SIZE)
    maps = []
    for k, crop in enumerate(crops_of(tr, GRID)):
        s, t = planted(k)
        maps.append(((crop - t) / s).float())
    return tuple(maps), tr.float(), tr


# ------------------------------------------------------------------------------------------------ the edge cases, by name
def _grid_of(size, ch, cw, ry, rx):
    return Grid(tuple(starts(size[0], ch, ry)), tuple(starts(size[1], cw, rx)), ch, cw, ry, rx)


# name -> (size (H, W), grid, the tiles' network size, the anchor's network size)
CASES = {
    "parity": (SIZE, GRID, NET, ANCHOR_NET),                                        # 3 x 3 tiles, a real resize on both axes
    "three_cover": ((43, 43), _grid_of((43, 43), 24, 24, 6, 6), (16, 16), (20, 20)),  # the 683-pixel rule scaled down: starts 0, 10, 19
    "ramp0": ((43, 70), _grid_of((43, 70), 24, 24, 0, 0), (16, 16), (20, 28)),
    "one_wide": ((50, 1), _grid_of((50, 1), 24, 1, 6, 0), (16, 4), (20, 4)),
    "one_high": ((1, 131), _grid_of((1, 131), 1, 24, 0, 6), (4, 16), (4, 40)),
    "grid64": ((260, 260), Grid(tuple(range(0, 253, 4)), tuple(range(0, 253, 4)), 8, 8, 4, 4), (8, 8), (36, 36)),   # 4096 tiles
}
assert CASES["three_cover"][1].xs == (0, 10, 19) and len(CASES["grid64"][1].ys) == 64 and CASES["grid64"][1].ys[-1] + 8 == 260
assert len(CASES["one_high"][1].xs) > 2 and len(CASES["ramp0"][1].xs) == 3


@functools.lru_cache(maxsize=None)
def case_maps(name):
    """-> (normal tiles, depth tiles, anchor) of CASES[name]"""
    size, grid, net, anchor_net = CASES[name]
    if name == "parity":
        return (normal_case(),) + depth_case()
    return (normal_case(grid, net, seed=len(name)),) + depth_case(grid, size, net, anchor_net)


@functools.lru_cache(maxsize=None)
def case_reference(name, normals=True):
    """-> dict: n64 / n32 (encoded [3,H,W]) and e_n; d64, c64, e_d, e_c (aligned); u64 and e_u (unaligned)"""
    size, grid, _, _ = CASES[name]
    nm, dm, anchor = case_maps(name)
    ref = {}
    if normals:
        ref["n64"] = blend_normals_restatement(nm, grid, size, torch.float64)
        ref["n32"] = blend_normals_restatement(nm, grid, size, torch.float32)
        ref["e_n"] = float((ref["n32"].double() - ref["n64"]).abs().max())
    ref["d64"], ref["c64"] = blend_depth_restatement(dm, grid, size, anchor, torch.float64)
    d32, c32 = blend_depth_restatement(dm, grid, size, anchor, torch.float32)
    ref["e_d"], ref["e_c"] = float((d32.double() - ref["d64"]).abs().max()), float((c32.double() - ref["c64"]).abs().max())
    return ref


def make_grid(grid, net, offset, anchor_offset=-1, anchor_net=(0, 0)):
    """-> preprocess.TileGrid of a Grid whose tiles start `offset` bytes into the maps"""
    from omnidata_amd import preprocess as pp
    return pp.TileGrid.make(offset, net, (grid.ch, grid.cw), grid.ys, grid.xs, (grid.ry, grid.rx), anchor_offset, anchor_net)


def pack_tiles(images):
    """images: [(tile maps, Grid, anchor map or None)] -> (one flat fp32 tensor: per image its tiles in grid order, then its
    anchor; [TileGrid] with the offsets into it)"""
    chunks, grids, off = [], [], 0
    for maps, grid, anchor in images:
        first = off
        for m in maps:
            chunks.append(m.reshape(-1))
            off += m.numel()
        a_off, a_net = -1, (0, 0)
        if anchor is not None:
            a_off, a_net = 4 * off, tuple(anchor.shape)
            chunks.append(anchor.reshape(-1))
            off += anchor.numel()
        grids.append(make_grid(grid, tuple(maps[0].shape[-2:]), 4 * first, a_off, a_net))
    return torch.cat(chunks).float().contiguous(), grids
