"""The cases and bounds that the device build (tests/test_gpu_tiled.py) and the host build under the sanitizers
(tests/test_tiled_cpu_build.py) of csrc/tiles.hip share.  Both hand in a runner R with two calls over raw buffers:
    R.normals(flat, grids, descs, total_bytes, mode)  -> the packed output as a uint8 tensor [total_bytes] on the host
    R.depth(flat, grids, descs, total_bytes, align)   -> (that, coeffs [tiles, 2] fp32 on the host; untouched rows with align=False)
flat: one fp32 host tensor with every map; grids: [preprocess.TileGrid]; descs: ctypes array of preprocess.ImageDesc.
A buffer is filled with the byte 0xA5 before the call, so what a call did not write is recognisable."""
import torch

from omnidata_amd import preprocess as pp
from tiled_restatement import (CASES, GRID, SIZE, blend_depth_restatement, blend_normals_restatement, case_maps, case_reference,
                               crops_of, pack_tiles, planted_case, seam_case, to_u8, u8_differences)

NORMAL_U8, NORMAL_F32, DEPTH_F32 = 1, 2, 3
BOUND_ABS = 2e-6            # the project's bound for a bilinear resize (tests/test_gpu_fullframe.py)
FILL = 0xA5


def _f32(raw, d, H, W, planes):
    return raw[d.offset:d.offset + 4 * planes * H * W].clone().view(torch.float32).view(*((planes, H, W) if planes > 1 else (H, W)))


def normals(R, images, sizes, output="f32", raw_views=False):
    """images: [(maps, Grid)] -> list of host tensors, [3,H,W] fp32 or [H,W,3] uint8"""
    flat, grids = pack_tiles([(m, g, None) for m, g in images])
    descs, total = pp.output_layout(sizes, "normal_u8" if output == "u8" else "normal_f32")
    mode = (NORMAL_U8 if output == "u8" else NORMAL_F32) | (pp.TTA_RAW_VIEWS if raw_views else 0)
    raw = R.normals(flat, grids, descs, max(total, 16), mode)
    if output == "u8":
        return [raw[d.offset:d.offset + 3 * H * W].clone().view(H, W, 3) for d, (H, W) in zip(descs, sizes)]
    return [_f32(raw, d, H, W, 3) for d, (H, W) in zip(descs, sizes)]


def depth(R, images, sizes, align=True):
    """images: [(maps, Grid, anchor or None)] -> ([H,W] fp32 host tensors, coeffs [tiles, 2] or None)"""
    flat, grids = pack_tiles(images)
    descs, total = pp.output_layout(sizes, "depth_f32")
    raw, coeffs = R.depth(flat, grids, descs, max(total, 16), align)
    return [_f32(raw, d, H, W, 1) for d, (H, W) in zip(descs, sizes)], (coeffs if align else None)


def _err(got, ref):
    return float((got.double() - ref).abs().max())


def check_case(R, name, report=print):
    """normals f32, depth f32 and the coefficients of CASES[name] within 2 e_ref + 2e-6 of the fp64 restatement; normals uint8
    within one level, at most 1 % of the bytes differing.  -> the figures"""
    size, grid, _, _ = CASES[name]
    nm, dm, anchor = case_maps(name)
    ref = case_reference(name)
    got_n = normals(R, [(nm, grid)], [size])[0]
    got_u = normals(R, [(nm, grid)], [size], "u8")[0]
    (got_d,), got_c = depth(R, [(dm, grid, anchor)], [size])
    err_n, err_d, err_c = _err(got_n, ref["n64"]), _err(got_d, ref["d64"]), _err(got_c, ref["c64"])
    worst, frac = u8_differences(got_u, to_u8(ref["n64"]))
    report(f"tiled parity {name} {size} {len(grid.ys)} x {len(grid.xs)} tiles: normals e_ref {ref['e_n']:.3e} err {err_n:.3e}; "
           f"depth e_ref {ref['e_d']:.3e} err {err_d:.3e}; coeffs e_ref {ref['e_c']:.3e} err {err_c:.3e}; "
           f"uint8 worst {worst} level(s), {frac:.2e} of the bytes differ")
    assert got_c.shape == ref["c64"].shape and got_d.shape == size and got_n.shape == (3, *size)
    assert err_n <= 2 * ref["e_n"] + BOUND_ABS, (name, err_n, ref["e_n"])
    assert err_c <= 2 * ref["e_c"] + BOUND_ABS, (name, err_c, ref["e_c"])
    assert err_d <= 2 * ref["e_d"] + BOUND_ABS, (name, err_d, ref["e_d"])
    assert worst <= 1 and frac <= 0.01, (name, worst, frac)
    return dict(err_n=err_n, err_d=err_d, err_c=err_c, worst=worst, frac=frac, **{k: v for k, v in ref.items() if k.startswith("e_")})


def check_unaligned_and_raw_views(R):
    """coeffs == NULL blends the tiles as they are; DPTX_TTA_RAW_VIEWS skips the normalisation at the network's resolution"""
    nm, dm, anchor = case_maps("parity")
    (got,), _ = depth(R, [(dm, GRID, None)], [SIZE], align=False)
    r64, _ = blend_depth_restatement(dm, GRID, SIZE, None, torch.float64, align=False)
    r32, _ = blend_depth_restatement(dm, GRID, SIZE, None, torch.float32, align=False)
    assert _err(got, r64) <= 2 * _err(r32, r64) + BOUND_ABS
    got = normals(R, [(nm, GRID)], [SIZE], raw_views=True)[0]
    r64 = blend_normals_restatement(nm, GRID, SIZE, torch.float64, normalize_views=False)
    r32 = blend_normals_restatement(nm, GRID, SIZE, torch.float32, normalize_views=False)
    assert _err(got, r64) <= 2 * _err(r32, r64) + BOUND_ABS
    assert _err(got, case_reference("parity")["n64"]) > 1e-4                              # the flag does something


def check_seam(R, report=print):
    """every tile the exact crop of one map: the blend is the map to 1e-6"""
    d, n = seam_case()
    (got_d,), _ = depth(R, [(crops_of(d, GRID), GRID, None)], [SIZE], align=False)
    got_n = normals(R, [(crops_of(n, GRID), GRID)], [SIZE], raw_views=True)[0]
    err_d, err_n = _err(got_d, 1 - d.double()), _err(got_n, n.double())
    report(f"tiled seam condition: depth {err_d:.3e} normals {err_n:.3e}")
    assert err_d <= 1e-6 and err_n <= 1e-6


def check_planted(R, report=print):
    """the planted case: aligned within 1e-5 of the truth, unaligned at least 1e-2 away"""
    maps, anchor, tr = planted_case()
    (aligned,), coeffs = depth(R, [(maps, GRID, anchor)], [SIZE])
    (plain,), _ = depth(R, [(maps, GRID, None)], [SIZE], align=False)
    e_a, e_p = _err(1 - aligned.double(), tr), _err(1 - plain.double(), tr)
    report(f"tiled planted case: aligned {e_a:.3e} unaligned {e_p:.3e}")
    assert e_a <= 1e-5 and e_p >= 1e-2
    return coeffs


def check_batch_and_reproducibility(R):
    """two images in one call equal two calls, and two runs are identical"""
    a, b = "three_cover", "parity"
    (sa, ga, _, _), (sb, gb, _, _) = CASES[a], CASES[b]
    (na, da, aa), (nb, db, ab) = case_maps(a), case_maps(b)
    for output in ("f32", "u8"):
        both = normals(R, [(na, ga), (nb, gb)], [sa, sb], output)
        again = normals(R, [(na, ga), (nb, gb)], [sa, sb], output)
        alone = normals(R, [(na, ga)], [sa], output) + normals(R, [(nb, gb)], [sb], output)
        assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(both, again, alone)), output
    both, cb = depth(R, [(da, ga, aa), (db, gb, ab)], [sa, sb])
    again, cb2 = depth(R, [(da, ga, aa), (db, gb, ab)], [sa, sb])
    (oa,), ca = depth(R, [(da, ga, aa)], [sa])
    (ob,), cb1 = depth(R, [(db, gb, ab)], [sb])
    assert torch.equal(both[0], oa) and torch.equal(both[1], ob) and torch.equal(cb, torch.cat([ca, cb1]))
    assert torch.equal(both[0], again[0]) and torch.equal(both[1], again[1]) and torch.equal(cb, cb2)


def check_canaries(R):
    """a uint8 output at an odd offset with rows 7 bytes longer than the pixels: no byte outside a row's own pixels is written;
    the same for fp32 rows 8 bytes longer"""
    size, grid, _, _ = CASES["parity"]
    H, W = size
    nm, dm, anchor = case_maps("parity")
    flat, grids = pack_tiles([(nm, grid, None)])
    tight = normals(R, [(nm, grid)], [size], "u8")[0]
    off, stride = 13, 3 * W + 7
    descs = (pp.ImageDesc * 1)(pp.ImageDesc(off, H, W, 3, stride))
    total = off + H * stride + 5
    raw = R.normals(flat, grids, descs, total, NORMAL_U8)
    rows = raw[off:off + H * stride].view(H, stride)
    assert torch.equal(rows[:, :3 * W].reshape(H, W, 3), tight)
    assert bool((raw[:off] == FILL).all()) and bool((raw[off + H * stride:] == FILL).all()) and bool((rows[:, 3 * W:] == FILL).all())
    flat, grids = pack_tiles([(dm, grid, anchor)])
    (tight_d,), _ = depth(R, [(dm, grid, anchor)], [size])
    off, stride = 16, 4 * W + 8
    descs = (pp.ImageDesc * 1)(pp.ImageDesc(off, H, W, 1, stride))
    total = off + H * stride + 4
    raw, _ = R.depth(flat, grids, descs, total, True)
    rows = raw[off:off + H * stride].view(H, stride)
    assert torch.equal(rows[:, :4 * W].clone().reshape(-1).view(torch.float32).view(H, W), tight_d)
    assert bool((raw[:off] == FILL).all()) and bool((raw[off + H * stride:] == FILL).all()) and bool((rows[:, 4 * W:] == FILL).all())


def check_non_finite(R):
    """NaN and infinities in one image's tiles (and its anchor) leave the other image of the call alone"""
    a, b = "three_cover", "parity"
    (sa, ga, _, _), (sb, gb, _, _) = CASES[a], CASES[b]
    (na, da, aa), (nb, db, ab) = case_maps(a), case_maps(b)
    bad = [float("nan"), float("inf"), -float("inf")]

    def poison(maps):
        maps = [m.clone() for m in maps]
        for k, m in enumerate(maps):
            m.view(-1)[k::7] = bad[k % 3]
        return tuple(maps)

    for output in ("f32", "u8"):
        got = normals(R, [(poison(na), ga), (nb, gb)], [sa, sb], output)
        assert torch.equal(got[1], normals(R, [(nb, gb)], [sb], output)[0])
    got, coeffs = depth(R, [(poison(da), ga, poison([aa])[0]), (db, gb, ab)], [sa, sb])
    (alone,), c_alone = depth(R, [(db, gb, ab)], [sb])
    assert torch.equal(got[1], alone) and torch.equal(coeffs[len(da):], c_alone)
