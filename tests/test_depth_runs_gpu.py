"""The depth trunk's run kernels -- depth_blk_kernel (csrc/depth_blk.hip: 32 x 32 maps with 128 / 32 channels, 16 x 16 with 256 / 64) and
depth_l3_kernel (csrc/igemm.hip: 8 x 8 with 512 / 128) -- through hcm_op_depth_run, against the float64 reference of the operation they perform
(tests/depth_run_cases.py block_ref).  The engines take these kernels only with the taps off, so no per-layer comparison with the oracle sees them.

Parity is PER BLOCK: the run of k blocks against block_ref applied to the device's own output of the run of k - 1 blocks, so that a rounding flip
in block j is not amplified through the later blocks (free-running, a correct float32 chain already differs from float64 by one storage ulp at
|ref| ~ 12 after four blocks: 7.8e-3 in fp16, 6.2e-2 in bf16).  Two elementwise conditions, both taken from the float32 CPU restatement of
block_ref (block_ref(..., dtype=torch.float32): on these inputs it reaches at most 0.87 of the first and 5.7 % in the second; each test prints
its figures beside the kernel's), none from the kernels:
    |got - ref| <= tol * max(1, |ref|) with tol of tests/test_ops_gpu.py's DT (fp16 3e-3, bf16 2e-2);
    at most 10 % of the elements differ from the reference at all.
Offset statistics (both kernels use the one-pass q / n - mean^2): the envelope DESIGN.md states for epilogue-fed statistics,
tests/test_norm_conditioning_gpu.py's _check16 at its CASES16.  Everything else holds to the bit.  profiles/depth_runs_parity.md has the figures."""
import ctypes as C

import pytest
import torch

from tests import depth_run_cases as dc
from tests.test_norm_conditioning_gpu import CASES16
from tests.test_ops_gpu import DT, _lib

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
MAX_SHARE = 0.10


def _bits(t):
    return t.contiguous().view(torch.int16)


class Dev:
    """a Run's parameters on the device, and launches of hcm_op_depth_run on them"""

    def __init__(self, run):
        self.run = run
        self.code, self.tdt, self.tol = DT[run.prec]
        self.w = [[t.cuda() for t in blk] for blk in run.w]
        self.gn = [[t.cuda() for t in blk] for blk in run.gn]
        self.width = run.groups * run.C

    def put(self, t, pad=0, fill=float("nan")):
        """t (B, HW, groups*C) -> device [B][HW][groups*C + pad], the pad columns holding `fill`"""
        d = torch.full((t.shape[0], t.shape[1], self.width + pad), fill, dtype=self.tdt, device="cuda")
        d[:, :, :self.width] = t.to(self.tdt).cuda()
        return d

    def call(self, x, y, n, first=0, ld=None, B=None, side=None, groups=None, code=None):
        """the raw entry on blocks first .. first + n - 1: returns its status"""
        r = self.run
        cnt = max(n, 1)
        blocks = [(self.w[(first + i) % r.nblocks], self.gn[(first + i) % r.nblocks], r.eps[(first + i) % r.nblocks]) for i in range(cnt)]
        w = (C.c_void_p * (3 * cnt))(*[t.data_ptr() for b in blocks for t in b[0]])
        gn = (C.c_void_p * (6 * cnt))(*[t.data_ptr() for b in blocks for t in b[1]])
        eps = (C.c_float * (3 * cnt))(*[e for b in blocks for e in b[2]])
        lib, _ = _lib()
        return lib.hcm_op_depth_run(x.data_ptr(), y.data_ptr(), w, gn, eps, self.code if code is None else code, x.shape[0] if B is None else B,
                                    r.side if side is None else side, r.groups if groups is None else groups, n, x.shape[2] if ld is None else ld,
                                    None)

    def launch(self, x, n, first=0):
        """blocks first .. first + n - 1 on x [B][HW][ld] into a fresh y: NaN where the kernel must write, SENTINEL in the pad columns, which
        must come back untouched; x must come back unchanged.  Returns y."""
        y = torch.full_like(x, float("nan"))
        y[:, :, self.width:] = SENTINEL
        before = _bits(x).clone()
        assert self.call(x, y, n, first) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(x), before), "the launch changed its input"
        assert bool((y[:, :, self.width:] == SENTINEL).all()), "the launch wrote into the pad columns"
        assert not bool(torch.isnan(y[:, :, :self.width]).any()), "the launch left output elements unwritten (or produced NaN)"
        return y


def _parity(run, pad, what, bound=None, variances_below_eps=()):
    """every k <= nblocks: the run of k blocks against block_ref on the device's output of the run of k - 1.  bound(ref) -> the absolute
    error bound of another rule than the two conditions (the offset cases).  Prints one line per block, asserts behind the last."""
    dev = Dev(run)
    x = dev.put(run.x, pad)
    prev, rows, bad = run.x, [], []
    for k in range(1, run.nblocks + 1):
        got = dev.launch(x, k)[:, :, :dev.width].cpu()
        var = [0.0, 0.0, 0.0]
        ref = dc.block_ref(prev, run.w[k - 1], run.gn[k - 1], run.eps[k - 1], dev.tdt, variances=var)
        r32 = dc.block_ref(prev, run.w[k - 1], run.gn[k - 1], run.eps[k - 1], dev.tdt, dtype=torch.float32)
        for i in variances_below_eps:          # the precondition of the low-variance cases, on the reference
            assert var[i] < run.eps[k - 1][i], (k, i, var[i], run.eps[k - 1][i])
        worst, share = dc.tolerance_stats(got, ref, dev.tol)
        w32, s32 = dc.tolerance_stats(r32, ref, dev.tol)
        line = (f"depth_run {what} side {run.side} [{run.prec}] B {run.B} groups {run.groups} pad {pad} block {k}/{run.nblocks}: "
                f"err/bound {worst:.3f} differing {100 * share:.2f} %  (float32 CPU: {w32:.3f}, {100 * s32:.2f} %)  max |ref| {ref.abs().max().item():.2f}")
        if variances_below_eps:
            line += "  conv group variances <= " + " ".join(f"{v:.1e}" for v in var) + "  eps " + " ".join(f"{e:.1e}" for e in run.eps[k - 1])
        if bound is not None:
            err, bnd = (got.double() - ref).abs().max().item(), bound(ref)
            line += f"  err {err:.3e}  bound {bnd:.3e}"
            if err > bnd:
                bad.append((k, err, bnd))
        elif worst > 1.0 or share > MAX_SHARE:
            bad.append((k, worst, share))
        print(line)
        rows.append((worst, share))
        prev = got
    assert not bad, bad
    return rows


# B, groups, pad columns: both batch sizes, both trunk counts, the dense and the padded row stride
LAYOUTS = [(1, 1, 0), (3, 2, 8), (1, 2, 8), (3, 1, 0)]


@pytest.mark.parametrize("B,groups,pad", LAYOUTS)
@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_id)
def test_every_block_of_a_run_matches_float64(case, B, groups, pad):
    """block counts 1 .. 4 (sides 32, 16) / 1 .. 6 (side 8), every block with its own weights, GroupNorm parameters and eps"""
    prec, side = case
    _parity(dc.make_run(side, prec, B, groups, dc.MAX_BLOCKS[side]), pad, "parity")


@pytest.mark.parametrize("low", [(0,), (0, 1, 2)], ids=["conv1", "all_convs"])
@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_id)
def test_eps_decides_a_low_variance_block(case, low):
    """Weights times 2^-8 (conv1's as the plain cases' eps is invisible: their group variances are about 0.2; with all three convs every
    GroupNorm of the block is eps-dominated): the group variances of those convs lie below their eps -- asserted on the reference --, where
    another eps moves the output by far more than the bound (tests/test_depth_runs_cpu.py).  Two blocks, so that block 1's eps is block 1's."""
    prec, side = case
    _parity(dc.make_run(side, prec, 2, 2, 2, low_variance=low), 0, "low-variance " + "+".join(f"conv{i + 1}" for i in low), variances_below_eps=low)


@pytest.mark.parametrize("ratio,prec", CASES16, ids=lambda v: str(v))
@pytest.mark.parametrize("side", [32, 16, 8])
def test_offset_statistics_of_conv1(side, ratio, prec):
    """block 0's conv1 output = noise + m with m = ratio x the noise's standard deviation (tests/test_norm_conditioning_gpu.py's _offset_conv):
    the one-pass variance q / n - mean^2 loses about ratio^2 of its float32 digits.  Bound: _check16's 4 x tol x max(1, max |ref|)."""
    run = dc.make_run(side, prec, 2, 2, 2, offset_ratio=ratio)
    tol = DT[prec][2]
    c1 = torch.stack([dc.conv1_out(run.x[:, :, g * run.C:(g + 1) * run.C], run.w[0][0][g], side) for g in range(2)])
    v = c1.reshape(-1, dc.GN_GROUPS, c1.shape[2] // dc.GN_GROUPS * side * side)
    print(f"depth_run offset side {side} ratio {ratio} [{prec}]: m {run.note['m']:.3f}  conv1 group |mean|/std "
          f"{(v.mean(-1).abs() / v.std(-1, unbiased=False)).max().item():.1f}")
    _parity(run, 8, f"offset ratio {ratio}", bound=lambda ref: 4 * tol * max(1.0, ref.abs().max().item()))


# ------------------------------------------------------------------------------------------------ what must hold to the bit
def _run(case, B=3, groups=2, n=None):
    prec, side = case
    return dc.make_run(side, prec, B, groups, n or dc.MAX_BLOCKS[side], seed=1)


@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_id)
def test_three_launches_give_the_same_bits(case):
    dev = Dev(_run(case))
    x = dev.put(dev.run.x)
    a, b, c = (dev.launch(x, dev.run.nblocks) for _ in range(3))
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c))


@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_id)
def test_a_sample_does_not_depend_on_its_place_in_the_batch(case):
    dev = Dev(_run(case))
    full = dev.launch(dev.put(dev.run.x), dev.run.nblocks)
    for b in range(dev.run.B):
        one = dev.launch(dev.put(dev.run.x[b:b + 1]), dev.run.nblocks)
        assert torch.equal(_bits(one[0]), _bits(full[b])), b


@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_id)
def test_a_trunk_of_a_pair_equals_the_trunk_alone(case):
    """trunk g of a groups = 2 launch against the groups = 1 launch on its slice of x and its own weights"""
    run = _run(case)
    dev = Dev(run)
    both = dev.launch(dev.put(run.x), run.nblocks)
    for g in range(2):
        solo = Dev(run.trunk(g))
        one = solo.launch(solo.put(solo.run.x), run.nblocks)
        assert torch.equal(_bits(one), _bits(both[:, :, g * run.C:(g + 1) * run.C])), g


@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_id)
def test_a_run_equals_its_blocks_launched_one_by_one(case):
    """the run of k blocks against block k launched alone on the run of k - 1's output, every k"""
    dev = Dev(_run(case))
    x = dev.put(dev.run.x)
    prev = x
    for k in range(1, dev.run.nblocks + 1):
        run_k = dev.launch(x, k)
        alone = dev.launch(prev, 1, first=k - 1)
        assert torch.equal(_bits(run_k), _bits(alone)), k
        prev = run_k


@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_id)
def test_a_padded_row_stride_gives_the_dense_bits(case):
    """ld = groups*C + 8: x's pad columns hold NaN (never read), y's the sentinel (never written: Dev.launch asserts it)"""
    dev = Dev(_run(case))
    dense = dev.launch(dev.put(dev.run.x), dev.run.nblocks)
    padded = dev.launch(dev.put(dev.run.x, 8), dev.run.nblocks)
    assert torch.equal(_bits(padded[:, :, :dev.width]), _bits(dense))


@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_id)
def test_in_place_where_the_kernel_allows_it(case):
    """Side 8: depth_l3_kernel copies its whole (sample, trunk) slice of x into LDS behind a barrier before anything else, keeps every block's
    output there and writes y once, at the end, the same slice -- so x == y is legal for any block count and must give the x != y bits.
    Sides 32 / 16: one block only (conv1 and the identity read a wave's own pixels, which only that wave stores, each channel slab after its
    identity rows have been read); more blocks in place are refused by the launcher (test_refusals)."""
    prec, side = case
    dev = Dev(_run(case))
    n = dev.run.nblocks if side == 8 else 1
    x = dev.put(dev.run.x, 8, SENTINEL)
    ref = dev.launch(x, n)
    assert dev.call(x, x, n) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(x), _bits(ref))


@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_id)
def test_refusals(case):
    """every bad argument returns non-zero and leaves a NaN-prefilled y untouched"""
    prec, side = case
    dev = Dev(_run(case))
    W, nmax = dev.width, dc.MAX_BLOCKS[side]
    x = dev.put(dev.run.x, 8)
    y = torch.full_like(x, float("nan"))
    bad = {"ld % 8": dict(ld=W + 4), "ld < groups*C": dict(ld=W - 8), "nblocks 0": dict(n=0), "nblocks beyond the kernel's": dict(n=nmax + 1),
           "a 32-bit dtype": dict(code=DT["fp32"][0]), "another side": dict(side=24), "side 0": dict(side=0), "no sample": dict(B=0), "no trunk": dict(groups=0)}
    for what, kw in bad.items():
        kw = dict(kw)
        assert dev.call(x, y, kw.pop("n", 2), **kw) != 0, what
    if side != 8:
        before = _bits(x).clone()
        assert dev.call(x, x, 2) != 0, "x == y with two blocks"
        torch.cuda.synchronize()
        assert torch.equal(_bits(x), before)
    lib, _ = _lib()
    assert lib.hcm_op_depth_run(x.data_ptr(), y.data_ptr(), None, None, None, dev.code, 3, side, 2, 1, W + 8, None) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())
    assert dev.call(x, y, 1) == 0          # ... and the same buffers are accepted when the arguments are right
    torch.cuda.synchronize()
    assert not bool(torch.isnan(y[:, :, :W]).any())
