"""Per-shape micro-benchmark of the implicit-GEMM kernel on the DPT-Hybrid layer shapes (B=32).
Usage (GPU box): python tools/gemm_bench.py [--dtype bf16]
                 python tools/gemm_bench.py --ab-flags 0,8 --gn --reps 5 --only s0.c3,s1.c3   (A/B of two launch forms)
                 python tools/gemm_bench.py --ab-gn-fold --reps 5 --iters 20 [--batch 16]      (conv3 + norm3: unfused vs folded)
                 python tools/gemm_bench.py --ab-stem --reps 5 --iters 20 [--batch 16]         (stem convolution: first vs second form)
                 python tools/gemm_bench.py --ab-upsample --reps 5 --iters 20 [--batch 16]     (x2 up-sampling: first form vs strips)"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omnidata_amd.engine import DTYPES, load_library  # noqa: E402

B = 32
DENSE = [("vit.qkv", B * 577, 2304, 768), ("vit.proj", B * 577, 768, 768), ("vit.fc1", B * 577, 3072, 768),
         ("vit.fc2", B * 577, 768, 3072), ("stem.gemm", B * 36864, 64, 192), ("patch.proj", B * 576, 768, 1024),
         # calibration against the square-GEMM figures of the CDNA4 programming guide (not DPT shapes; --only cal.4096,...)
         ("cal.4096", 4096, 4096, 4096), ("cal.8192", 8192, 8192, 8192)]
# name, H, Cin, Cout, k, stride, pad, Ho
CONV = [("rcu@96", 96, 256, 256, 3, 1, 1, 96), ("rcu@48", 48, 256, 256, 3, 1, 1, 48), ("rcu@24", 24, 256, 256, 3, 1, 1, 24),
        ("rcu@12", 12, 256, 256, 3, 1, 1, 12), ("head.0", 192, 256, 128, 3, 1, 1, 192), ("head.2", 384, 128, 32, 3, 1, 1, 384),
        ("l2_rn", 48, 512, 256, 3, 1, 1, 48), ("l3_rn", 24, 768, 256, 3, 1, 1, 24), ("out_conv@96", 96, 256, 256, 1, 1, 0, 96),
        ("s0.c1", 96, 256, 64, 1, 1, 0, 96), ("s0.c2", 96, 64, 64, 3, 1, 1, 96), ("s0.c3", 96, 64, 256, 1, 1, 0, 96),
        ("s1.c1", 48, 512, 128, 1, 1, 0, 48), ("s1.c2", 48, 128, 128, 3, 1, 1, 48), ("s1.c3", 48, 128, 512, 1, 1, 0, 48),
        ("s2.c1", 24, 1024, 256, 1, 1, 0, 24), ("s2.c2", 24, 256, 256, 3, 1, 1, 24), ("s2.c3", 24, 256, 1024, 1, 1, 0, 24),
        ("s1.b0.c2(s2)", 96, 128, 128, 3, 2, 0, 48), ("pp4.conv2", 24, 768, 768, 3, 2, 1, 12),
        # the remaining small-K 1x1 launches of the stages and the decoder (s0.ds has s0.c3's shape)
        ("s0.c1a", 96, 64, 64, 1, 1, 0, 96), ("s1.b0.c1", 96, 256, 128, 1, 1, 0, 96), ("s1.ds", 96, 256, 512, 1, 2, 0, 48),
        ("out_conv@48", 48, 256, 256, 1, 1, 0, 48), ("out_conv@24", 24, 256, 256, 1, 1, 0, 24), ("out_conv@12", 12, 256, 256, 1, 1, 0, 12)]


ITERS = [10]


def timeit(fn, iters=None):
    iters = iters or ITERS[0]
    return _timeit(fn, iters)


def _timeit(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def ab_conv(lib, dt, tdt, st, args, only):
    """Alternating A/B of two dptx_debug_set_gemm_flags values on the 16-bit conv shapes: --reps repetitions of --iters launches
    per side, interleaved; prints every repetition, the medians and each side's spread (max - min).  --gn: the stage convs
    run as the forward runs them, with the GroupNorm records written by the epilogue -- dptx_op_conv_groupnorm, i.e. the conv
    plus the apply pass, which is the same on both sides (out_conv has a bias instead and is timed alone)."""
    fa, fb = [int(v) for v in args.ab_flags.split(",")]
    print(f"# flags {fa} vs {fb}, {args.reps} x {args.iters} launches, B = {B}, records {'on' if args.gn else 'off'}; us per launch")
    for name, H, Cin, Cout, k, s, pad, Ho in CONV:
        if only and name not in only:
            continue
        X = torch.randn(B, H, H, Cin, device="cuda").to(tdt)
        Wt = (torch.randn(Cout, k, k, Cin, device="cuda") * (k * k * Cin) ** -0.5).to(tdt)
        Y, Y2 = torch.empty(B, Ho, Ho, Cout, device="cuda", dtype=tdt), torch.empty(B, Ho, Ho, Cout, device="cuda", dtype=tdt)
        bias, g = torch.randn(Cout, device="cuda"), torch.randn(Cout, device="cuda")
        gn = args.gn and not name.startswith("out_conv") and (Ho * Ho) % 32 == 0 and Cout % 64 == 0
        rec = torch.zeros(B * (Ho * Ho // 32 + 1) * 64, device="cuda")
        if gn:
            fn = lambda: lib.dptx_op_conv_groupnorm(dt, X.data_ptr(), Wt.data_ptr(), Y.data_ptr(), g.data_ptr(), bias.data_ptr(), None,
                                                    Y2.data_ptr(), B, H, H, Cin, Cout, k, s, pad, pad, Ho, Ho, 1, 1e-5, rec.data_ptr(), st)
        else:
            fn = lambda: lib.dptx_op_conv(dt, X.data_ptr(), Wt.data_ptr(), bias.data_ptr(), None, Y.data_ptr(), B, H, H, Cin, Cout,
                                          k, s, pad, pad, Ho, Ho, 0, 0, st)
        t = {fa: [], fb: []}
        try:
            for _ in range(args.reps):
                for f in (fa, fb):
                    lib.dptx_debug_set_gemm_flags(f)
                    t[f].append(timeit(fn) * 1e3)
        finally:
            lib.dptx_debug_set_gemm_flags(0)
        med = {f: sorted(v)[len(v) // 2] for f, v in t.items()}
        spr = {f: max(v) - min(v) for f, v in t.items()}
        print(f"{name:12s} K={k * k * Cin:4d} N={Cout:4d} s={s} {'conv+gn' if gn else 'conv   '}  flag{fa} " + " ".join(f"{v:6.1f}" for v in t[fa]) +
              f"  | flag{fb} " + " ".join(f"{v:6.1f}" for v in t[fb]) +
              f"  | median {med[fa]:6.1f} vs {med[fb]:6.1f}  delta {med[fb] - med[fa]:+6.1f}  spread {spr[fa]:4.1f} / {spr[fb]:4.1f}")
        del X, Wt, Y, Y2


def ab_gn_fold(lib, dt, tdt, st, args, only):
    """conv3 + norm3 of the three stage classes, with shortcut and ReLU as the later blocks of a stage run them: conv + apply pass
    (dptx_op_conv_groupnorm on the forward's dispatch) against statistics pass + finalize + GroupNorm-epilogue pass
    (dptx_op_conv_groupnorm_fused), alternating, --reps repetitions of --iters calls per side; then the statistics pass and the
    finalize launch alone.  Prints every repetition, the medians, each side's spread (max - min) and the verdict of the adoption
    rule: the folded side is faster by more than the larger spread."""
    print(f"# conv3 + norm3 unfused vs folded, {args.reps} x {args.iters} calls, B = {B}, {args.dtype}; us per call")
    for name, H, Cin, Cout, k, s, pad, Ho in CONV:
        if name not in ("s0.c3", "s1.c3", "s2.c3") or (only and name not in only):
            continue
        X = torch.randn(B, H, H, Cin, device="cuda").to(tdt)
        Wt = (torch.randn(Cout, 1, 1, Cin, device="cuda") * Cin ** -0.5).to(tdt)
        R = torch.randn(B, H, H, Cout, device="cuda").to(tdt)
        Yraw, Y = torch.empty_like(R), torch.empty_like(R)
        beta, g = torch.randn(Cout, device="cuda"), torch.randn(Cout, device="cuda")
        rec = torch.zeros(B * (H * H // 32 + 1) * 64, device="cuda")
        tab = torch.zeros(B * 4 * Cout, device="cuda")

        def fused(passes):
            return lambda: lib.dptx_op_conv_groupnorm_fused(dt, X.data_ptr(), Wt.data_ptr(), g.data_ptr(), beta.data_ptr(), R.data_ptr(), None,
                                                            None, None, Y.data_ptr(), B, H, H, Cin, Cout, 1, 1e-5, rec.data_ptr(),
                                                            tab.data_ptr(), passes, st)
        sides = {"unfused": lambda: lib.dptx_op_conv_groupnorm(dt, X.data_ptr(), Wt.data_ptr(), Yraw.data_ptr(), g.data_ptr(), beta.data_ptr(),
                                                               R.data_ptr(), Y.data_ptr(), B, H, H, Cin, Cout, 1, 1, 0, 0, H, H, 1, 1e-5,
                                                               rec.data_ptr(), st),
                 "folded": fused(7)}
        assert sides["unfused"]() == 0 and sides["folded"]() == 0
        t = {n: [] for n in sides}
        for _ in range(args.reps):
            for n, fn in sides.items():
                t[n].append(timeit(fn) * 1e3)
        med = {n: sorted(v)[len(v) // 2] for n, v in t.items()}
        spr = {n: max(v) - min(v) for n, v in t.items()}
        gain = med["unfused"] - med["folded"]
        print(f"{name:6s} K={Cin:4d} N={Cout:4d}  unfused " + " ".join(f"{v:6.1f}" for v in t["unfused"]) + "  | folded " +
              " ".join(f"{v:6.1f}" for v in t["folded"]) + f"  | median {med['unfused']:6.1f} vs {med['folded']:6.1f}  gain {gain:+6.1f}"
              f"  spread {spr['unfused']:4.1f} / {spr['folded']:4.1f}  -> {'faster' if gain > max(spr.values()) else 'not faster'}")
        parts = {"stats": fused(1), "finalize": fused(2), "epilogue": fused(4)}
        tp = {n: sorted(timeit(fn) * 1e3 for _ in range(args.reps)) for n, fn in parts.items()}
        a_mb = B * H * H * Cin * 2 / 1e6
        print(f"{'':6s} alone: " + "  ".join(f"{n} {v[len(v) // 2]:6.1f} ({v[0]:.1f} .. {v[-1]:.1f})" for n, v in tp.items()) +
              f"   [statistics pass reads A = {a_mb:.1f} MB: {a_mb / tp['stats'][len(tp['stats']) // 2]:.2f} TB/s]")
        del X, Wt, R, Yraw, Y


def _ab(sides, args):
    """alternating --reps repetitions of --iters launches per side -> ({side: [us]}, {side: median}, {side: max - min})"""
    for fn in sides.values():
        assert fn() == 0
    t = {n: [] for n in sides}
    for _ in range(args.reps):
        for n, fn in sides.items():
            t[n].append(timeit(fn) * 1e3)
    return t, {n: sorted(v)[len(v) // 2] for n, v in t.items()}, {n: max(v) - min(v) for n, v in t.items()}


def _flagged(lib, flag, fn):
    def run():
        lib.dptx_debug_set_gemm_flags(flag)
        try:
            return fn()
        finally:
            lib.dptx_debug_set_gemm_flags(0)
    return run


def ab_stem(lib, dt, tdt, st, args):
    """The stem convolution at 384 x 384 from an fp32 image: stem_conv_kernel (debug flag 128) against stem_conv_kernel_wp (the
    dispatch), alternating; every repetition, the medians, each side's spread and the verdict of the adoption rule (faster by
    more than the larger spread); bytes the launch has to move (image in + raw map out) over the median = achieved TB/s."""
    print(f"# stem conv 384 x 384, old (flag 128) vs new, {args.reps} x {args.iters} launches, B = {B}, {args.dtype}; us per launch")
    x = torch.rand(B, 3, 384, 384, device="cuda")
    Wt = (torch.randn(64, 176, device="cuda") * 147 ** -0.5).to(tdt)
    y = torch.empty(B, 192, 192, 64, device="cuda", dtype=tdt)
    call = lambda: lib.dptx_op_stem_conv(dt, x.data_ptr(), Wt.data_ptr(), y.data_ptr(), B, 384, 384, st)
    t, med, spr = _ab({"old": _flagged(lib, 128, call), "new": call}, args)
    mb = (x.numel() * 4 + y.numel() * 2) / 1e6
    gain = med["old"] - med["new"]
    print("stem  old " + " ".join(f"{v:6.1f}" for v in t["old"]) + "  | new " + " ".join(f"{v:6.1f}" for v in t["new"]) +
          f"  | median {med['old']:6.1f} vs {med['new']:6.1f}  gain {gain:+6.1f}  spread {spr['old']:4.1f} / {spr['new']:4.1f}"
          f"  -> {'faster' if gain > max(spr.values()) else 'not faster'}")
    print(f"      {mb:.1f} MB in + out: old {mb / med['old']:.2f} TB/s, new {mb / med['new']:.2f} TB/s")


def ab_upsample(lib, dt, tdt, st, args):
    """The four decoder up-samplings (C = 256): upsample2x_kernel (debug flag 128) against the strip form with 4 and with 8
    output rows per thread, alternating; medians, spreads, the adoption rule per strip height, and bytes written over the
    median = achieved write rate."""
    print(f"# x2 up-sampling C = 256, old (flag 128) vs strips of 4 / 8 rows, {args.reps} x {args.iters} launches, B = {B}, {args.dtype}; us per launch")
    for H in (96, 48, 24, 12):
        X = torch.randn(B, H, H, 256, device="cuda").to(tdt)
        Y = torch.empty(B, 2 * H, 2 * H, 256, device="cuda", dtype=tdt)
        old = lambda: lib.dptx_op_upsample2x(dt, X.data_ptr(), Y.data_ptr(), B, H, H, 256, st)
        strip = lambda R: (lambda: lib.dptx_op_upsample2x_strip(dt, X.data_ptr(), Y.data_ptr(), B, H, H, 256, R, st))
        t, med, spr = _ab({"old": _flagged(lib, 128, old), "strip4": strip(4), "strip8": strip(8)}, args)
        out_mb = Y.numel() * 2 / 1e6
        line = f"up@{H:<3d} " + "  | ".join(f"{n} " + " ".join(f"{v:6.1f}" for v in t[n]) for n in t) + "  | median " + \
            " / ".join(f"{med[n]:6.1f}" for n in t) + "  spread " + " / ".join(f"{spr[n]:4.1f}" for n in t)
        for n in ("strip4", "strip8"):
            gain = med["old"] - med[n]
            line += f"  {n} gain {gain:+6.1f} -> {'faster' if gain > max(spr['old'], spr[n]) else 'not faster'}"
        print(line)
        print(f"        writes {out_mb:.1f} MB: " + ", ".join(f"{n} {out_mb / med[n]:.2f} TB/s" for n in t))
        del X, Y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--only", default=None, help="comma separated shape names")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32, help="images (conv shapes only): 16 = what one of the two streams launches")
    ap.add_argument("--ab-flags", default=None, help="two dptx_debug_set_gemm_flags values, e.g. 0,8: alternating A/B on the conv shapes")
    ap.add_argument("--reps", type=int, default=5, help="repetitions per side of --ab-flags")
    ap.add_argument("--ab-gn-fold", action="store_true",
                    help="conv3 + norm3 of the three stage classes: conv + apply pass vs statistics + finalize + GroupNorm-epilogue pass")
    ap.add_argument("--ab-stem", action="store_true", help="stem convolution: stem_conv_kernel (flag 128) vs stem_conv_kernel_wp")
    ap.add_argument("--ab-upsample", action="store_true", help="x2 up-sampling of the four decoder classes: first form vs strips of 4 / 8 rows")
    ap.add_argument("--gn", action="store_true", help="--ab-flags: GroupNorm records on (conv + apply pass) where the forward has them")
    args = ap.parse_args()
    global B
    B = args.batch
    only = set(args.only.split(",")) if args.only else None
    ITERS[0] = args.iters
    lib = load_library()  # builds the library first if it is missing or stale
    fp8 = args.dtype == "fp8"
    dt, tdt = DTYPES[args.dtype], (torch.bfloat16 if args.dtype in ("bf16", "fp8") else torch.float16)
    st = torch.cuda.current_stream().cuda_stream
    if args.ab_gn_fold:
        return ab_gn_fold(lib, dt, tdt, st, args, only)
    if args.ab_stem or args.ab_upsample:
        if args.ab_stem:
            ab_stem(lib, dt, tdt, st, args)
        if args.ab_upsample:
            ab_upsample(lib, dt, tdt, st, args)
        return
    if args.ab_flags:
        return ab_conv(lib, dt, tdt, st, args, only)
    tot_ms, tot_flop = 0.0, 0.0
    # the ViT GEMMs run with the epilogue the engine gives them: fc1 bias + GELU; proj / fc2 bias + in-place fp32 residual
    EPI = {"vit.fc1": (2, False), "vit.proj": (0, True), "vit.fc2": (0, True)}
    for name, M, N, K in DENSE:
        if (only and name not in only) or fp8 or (name.startswith("cal.") and not only):
            continue
        act, inplace32 = EPI.get(name, (0, False))
        A = torch.randn(M, K, device="cuda").to(tdt)
        W = (torch.randn(N, K, device="cuda") * K ** -0.5).to(tdt)
        C = torch.zeros(M, N, device="cuda", dtype=torch.float32 if inplace32 else tdt)
        bias = torch.randn(N, device="cuda") * (0.0 if inplace32 else 1.0)
        R = C.data_ptr() if inplace32 else None
        ms = timeit(lambda: lib.dptx_op_gemm(dt, A.data_ptr(), W.data_ptr(), bias.data_ptr(), R, C.data_ptr(), M, N, K, act, 0,
                                             int(inplace32), int(inplace32), st))
        fl = 2.0 * M * N * K
        print(f"{name:14s} M={M:8d} N={N:5d} K={K:5d}  {ms:8.3f} ms  {fl / ms / 1e9:8.1f} TF/s")
        tot_ms += ms; tot_flop += fl
    if fp8:  # the ViT linears on the e4m3 kernel (DPTX_FLAG_FP8_VIT): a dense GEMM is a 1x1 convolution over a 577 x 1 "image"
        for name, M, N, K in DENSE:
            if (only and name not in only) or not name.startswith("vit.") or name == "vit.proj":
                continue
            X = torch.randn(B, 577, 1, K, device="cuda").to(torch.float8_e4m3fn)
            Wt = (torch.randn(N, 1, 1, K, device="cuda") * 16.0).to(torch.float8_e4m3fn)
            Y = torch.empty(B, 577, 1, N, device="cuda", dtype=tdt)
            Y8 = torch.empty(B, 577, 1, N, device="cuda", dtype=torch.uint8)
            bias = torch.randn(N, device="cuda")
            act = 2 if name == "vit.fc1" else 0
            ms = timeit(lambda: lib.dptx_op_conv_fp8(X.data_ptr(), Wt.data_ptr(), bias.data_ptr(), None, Y.data_ptr(), Y8.data_ptr(), B, 577, 1,
                                                     K, N, 1, 1, 0, 0, 577, 1, act, 0, 1.0 / 768, st))
            fl = 2.0 * B * 577 * N * K
            print(f"{name + '@fp8':14s} M={B * 577:8d} N={N:5d} K={K:5d}  {ms:8.3f} ms  {fl / ms / 1e9:8.1f} TF/s")
            tot_ms += ms; tot_flop += fl
    for name, H, Cin, Cout, k, s, pad, Ho in CONV:
        if only and name not in only:
            continue
        if fp8 and Cin % 128:
            continue
        X = torch.randn(B, H, H, Cin, device="cuda").to(torch.float8_e4m3fn if fp8 else tdt)
        Wt = (torch.randn(Cout, k, k, Cin, device="cuda") * (16.0 if fp8 else (k * k * Cin) ** -0.5)).to(torch.float8_e4m3fn if fp8 else tdt)
        Y = torch.empty(B, Ho, Ho, Cout, device="cuda", dtype=tdt)
        bias = torch.randn(Cout, device="cuda")
        if fp8:  # the fp8 dtype's convolution: e4m3 operands, bf16 output + e4m3 copy of it
            Y8 = torch.empty(B, Ho, Ho, Cout, device="cuda", dtype=torch.uint8)
            ms = timeit(lambda: lib.dptx_op_conv_fp8(X.data_ptr(), Wt.data_ptr(), bias.data_ptr(), None, Y.data_ptr(), Y8.data_ptr(), B, H,
                                                     H, Cin, Cout, k, s, pad, pad, Ho, Ho, 0, 0, 1.0 / 768, st))
        else:
            ms = timeit(lambda: lib.dptx_op_conv(dt, X.data_ptr(), Wt.data_ptr(), bias.data_ptr(), None, Y.data_ptr(), B, H, H, Cin, Cout,
                                                 k, s, pad, pad, Ho, Ho, 0, 0, st))
        M, K = B * Ho * Ho, k * k * Cin
        fl = 2.0 * M * Cout * K
        print(f"{name:14s} M={M:8d} N={Cout:5d} K={K:5d}  {ms:8.3f} ms  {fl / ms / 1e9:8.1f} TF/s")
        tot_ms += ms; tot_flop += fl
        del X, Wt, Y
    print(f"TOTAL {tot_ms:.3f} ms  {tot_flop / tot_ms / 1e9:.1f} TF/s (unweighted list)")


if __name__ == "__main__":
    main()
