"""The attention kernel (csrc/attention.hip) judged row by row: every output element against the fp64 attention of the same
rounded operands, with tests/gpu_util.attention_row_bound as the bar -- a bound per (image, head, query, d) that follows the
rounding steps of the kernel, and that tests/test_attention_host.py shows to be met by a correct kernel and missed by one that
lets a key too many through, drops the last key, counts key 0 twice, mixes heads or images, or forgets to rescale l.

Matrix: bf16 / fp16 / bf16x3 / fp16x3 x three input families x ten (B, S, H) with 12 and 16 heads: S = 1 (no key tile), 2,
17, 65 (the last tile holds one key beyond the first), 128 (63 keys in the last tile), 129 (two tiles exactly, a second query
block of one row), 193 (three tiles exactly), 321 and 505 (flex lengths) and 577.  Besides the bound: nothing is written
behind row B * S, every row before it is written, a second launch is bit-identical, and no (image, head) sees another one's
Q, K or V.  Run on an MI355X: pytest -m gpu."""
import functools

import pytest
import torch

from omnidata_amd.engine import DTYPES, load_library
from tests.gpu_util import (ATT_FAMILIES, ATT_MODES, ATT_PLANES, ATT_SHAPES, PlaneArena, attention_inputs, attention_ref64,
                            attention_row_bound, ptr, stream)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 128          # rows behind B * S, inside the test's own tensor, that must stay untouched
SENTINEL = 0x7FED  # a NaN in bf16 and in fp16: the kernel never writes it


def shape_id(s):
    return "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def inputs(shape, family):
    """fp32 CPU inputs of one case, shared by the four modes and by the tests below; never modified (clone first)"""
    return attention_inputs(*shape, family)


class AttentionRun:
    """qkv (rounded to the mode's planes) and an output of B * S + PAD rows on the device; launch() prefills the output with
    SENTINEL, runs dptx_op_attention and returns the bits of the hi plane and of the lo plane (None for bf16 / fp16)."""

    def __init__(self, mode, x):
        self.mode, (self.dt, self.pl) = mode, ATT_PLANES[mode]
        self.B, self.S, _, self.H, _ = x.shape
        B, S, H = self.B, self.S, self.H
        self.ar = None
        if self.pl == 2:
            self.ar = PlaneArena(x.numel() + (B * S + PAD) * H * 64 + 4096, dtype=self.dt)
            self.qkv = self.ar.put(x.reshape(B * S, 3 * H * 64))
            self.out = self.ar.empty(B * S + PAD, H * 64)
            self.out_lo = self.ar.lo(self.out)
            self.val = self.ar.value(self.qkv).view(B, S, 3, H, 64)
        else:
            self.qkv = x.to(DEV).to(self.dt).reshape(B * S, 3 * H * 64).contiguous()
            self.out = torch.empty(B * S + PAD, H * 64, device=DEV, dtype=self.dt)
            self.out_lo = None
            self.val = self.qkv.double().view(B, S, 3, H, 64)

    def launch(self):
        planes = [self.out] + ([self.out_lo] if self.pl == 2 else [])
        for t in planes:
            t.view(torch.int16).fill_(SENTINEL)
        rc = load_library().dptx_op_attention(DTYPES[self.mode], ptr(self.qkv), ptr(self.out), self.B, self.S, self.H, stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        bits = [t.view(torch.int16).clone() for t in planes]
        return bits[0], (bits[1] if self.pl == 2 else None)

    def value(self, hi_bits, lo_bits):
        """fp64 value [B, S, H, 64] of the first B * S rows"""
        n = self.B * self.S
        v = hi_bits[:n].view(self.dt).double()
        if lo_bits is not None:
            v = v + lo_bits[:n].view(self.dt).double()
        return v.view(self.B, self.S, self.H, 64)

    def close(self):
        if self.ar is not None:
            self.ar.release()


def ratio_to_bound(run, hi_bits, lo_bits):
    """|out - o| / bound elementwise [B, S, H, 64]; a bound of 0 (S = 1: the output is v0 exactly) admits no error"""
    o, A, l, Vsum = attention_ref64(run.val)
    err = (run.value(hi_bits, lo_bits) - o).abs()
    bound = attention_row_bound(run.mode, A, l, Vsum).expand_as(err)
    return torch.where(err == 0, torch.zeros_like(err), err / bound)


def worst_of(ratio):
    i = int(ratio.argmax())
    B, S, H, D = ratio.shape
    return float(ratio.flatten()[i]), dict(b=i // (S * H * D), q=i // (H * D) % S, head=i // D % H, d=i % D)


@pytest.mark.parametrize("shape", ATT_SHAPES, ids=shape_id)
@pytest.mark.parametrize("family", ATT_FAMILIES)
@pytest.mark.parametrize("mode", ATT_MODES)
def test_attention_rows(mode, family, shape):
    B, S, H = shape
    run = AttentionRun(mode, inputs(shape, family))
    try:
        hi, lo = run.launch()
        # 1. every element within its own bound
        ratio = ratio_to_bound(run, hi, lo)
        assert not torch.isnan(ratio).any()
        worst, where = worst_of(ratio)
        print(f"\n[attention rows] {mode} {family} {shape_id(shape)}: worst |err| / bound {worst:.3f} at {where}")
        assert worst <= 1.0, f"{mode} {family} B={B} S={S} H={H}: |err| = {worst:.3f} x bound at {where}"
        # 2. rows >= B * S untouched, every row before them written (both planes)
        for name, bits in (("hi", hi), ("lo", lo)):
            if bits is None:
                continue
            assert bool((bits[B * S:] == SENTINEL).all()), f"{name} plane: written behind row B * S = {B * S}"
            unwritten = (bits[:B * S] == SENTINEL).view(B, S, H, 64).any(-1).nonzero()
            assert unwritten.numel() == 0, f"{name} plane: (b, q, head) never written: {unwritten[:8].tolist()}"
        # 3. a second launch gives the same bits
        hi2, lo2 = run.launch()
        assert torch.equal(hi, hi2) and (lo is None or torch.equal(lo, lo2)), "second launch differs"
    finally:
        run.close()


@pytest.mark.parametrize("shape", [(3, 129, 16), (2, 577, 12)], ids=shape_id)
@pytest.mark.parametrize("mode", ATT_MODES)
def test_attention_pairs_are_isolated(mode, shape):
    """replacing Q, K and V of ONE (image, head) changes that pair's output and not one bit of any other's"""
    B, S, H = shape
    x = inputs(shape, "peaked")
    other = attention_inputs(B, S, H, "lastkeys", seed=1)

    def bits_of(x_):
        run = AttentionRun(mode, x_)
        try:
            hi, lo = run.launch()
        finally:
            run.close()
        planes = [hi[:B * S]] + ([lo[:B * S]] if lo is not None else [])
        return torch.stack(planes).view(len(planes), B, S, H, 64)

    first = bits_of(x)
    for b0, h0 in ((B - 1, 5), (0, H - 1)):
        x2 = x.clone()
        x2[b0, :, :, h0] = other[b0, :, :, h0]
        differs = (bits_of(x2) != first).any(0).any(-1).any(1)    # [B, H]: any plane, any d, any query
        assert bool(differs[b0, h0]), f"(b, head) = ({b0}, {h0}) was replaced and its output did not change"
        differs[b0, h0] = False
        assert not bool(differs.any()), f"replacing (b, head) = ({b0}, {h0}) changed (b, head) {differs.nonzero().tolist()}"


@pytest.mark.parametrize("shape", [(3, 129, 16), (1, 321, 16)], ids=shape_id)
@pytest.mark.parametrize("mode", ATT_MODES)
def test_attention_query_block_edges(mode, shape):
    """the last row of the first 128-query block, the first row of the second one (at S = 129 its only row: 31 of the wave's 32
    lanes and three of the block's four waves have no query) and the last row of all, named one by one"""
    B, S, H = shape
    for family in ATT_FAMILIES:
        run = AttentionRun(mode, inputs(shape, family))
        try:
            ratio = ratio_to_bound(run, *run.launch())
        finally:
            run.close()
        for q in (127, 128, S - 1):
            worst, where = worst_of(ratio[:, q:q + 1])
            where["q"] = q
            assert worst <= 1.0, f"{mode} {family} S={S}: query row {q}: |err| = {worst:.3f} x bound at {where}"


@pytest.mark.parametrize("mode", ["fp16", "bf16x3", "fp16x3"])
def test_row_bound_sees_one_key_too_many_on_the_device(mode):
    """positive control of the whole chain (device reference, bound, comparison) at the longest sequence: the kernel run on
    S + 1 tokens, the last one a zero key with zero value -- what a mask that lets key S through would compute -- must MISS the
    bound of the S-token reference in the flat family (CPU model: 2.3 x, 25 x and 72 x the bound).  bf16 is absent on purpose:
    at S = 577 one key in 577 is below its rounding (0.74 of the bound)."""
    B, S, H = shape = (2, 577, 12)
    x = inputs(shape, "flat")
    run = AttentionRun(mode, torch.cat([x, torch.zeros(B, 1, 3, H, 64)], 1))
    try:
        got = run.value(*run.launch())[:, :S]
        o, A, l, Vsum = attention_ref64(run.val[:, :S])
    finally:
        run.close()
    worst = float(((got - o).abs() / attention_row_bound(mode, A, l, Vsum)).max())
    print(f"\n[attention rows] {mode} flat {shape_id(shape)} with a zero key appended: worst |err| / bound {worst:.2f}")
    assert worst > 1.0, worst
