"""Cases and the float64 reference for the depth trunk's run kernels (csrc/depth_blk.hip depth_blk_kernel, csrc/igemm.hip depth_l3_kernel), as
hcm_op_depth_run launches them.  CPU only, everything rebuilt from the seed.

A run is `nblocks` identity bottlenecks of habitat's GroupNorm ResNet-50 (oracle/hcm_oracle.py habitat_resnet_encoder, the block statements of its
inner loop without the down-sample branch): conv1x1 -> GroupNorm(16) -> ReLU -> conv3x3 pad 1 -> GroupNorm -> ReLU -> conv1x1 -> GroupNorm -> + x ->
ReLU, on `groups` trunks whose channels lie side by side in every pixel.  Layouts are the kernels' (csrc/kernels.h DepthBlk / DepthL3):
    x            (B, side*side, groups*C), trunk g at channels [g*C, +C)
    w1 w2 w3     [groups][CM][C], [groups][CM][9*CM] with k = tap*CM + ci, [groups][C][CM]
    gamma, beta  [groups*channels] float32, three pairs per block

The inputs: x non-negative (a block input is a ReLU output), weights uniform times sqrt(2 / fan-in) as tests/test_ops_gpu.py's
test_conv2d_groupnorm_fused draws them, gamma in [0.5, 1.5], beta in +-0.1, every block its own weights, and a DIFFERENT eps for every conv of every
block -- 1e-5 x {1, 4, 1/4}, the values the fp16 range fold produces (forward.cpp fill_run: 1e-5 x fold^2) -- so that a kernel that reads the wrong
block's or the wrong conv's parameters cannot pass."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

SHAPES = {32: (128, 32), 16: (256, 64), 8: (512, 128)}        # map side -> (C, CM): layer1, layer2 (depth_blk_kernel), layer3 (depth_l3_kernel)
MAX_BLOCKS = {32: 4, 16: 4, 8: 6}                             # the launchers' limits
GN_GROUPS = 16
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
EPS_FACTORS = (1.0, 4.0, 0.25)
# every template instantiation: 2 storage types x 3 shapes
CASES = [(prec, side) for prec in ("fp16", "bf16") for side in (32, 16, 8)]


def case_id(c):
    return f"{c[0]}-side{c[1]}"


def eps_of(blk, conv):
    """eps of conv `conv` (0..2) of block `blk`, as the float32 the C ABI carries: block 0's conv1 has 1e-5, no two convs of a block and no two
    neighbouring blocks share a value"""
    return float(np.float32(1e-5 * EPS_FACTORS[(blk + conv) % 3]))


class Run:
    """x (B, side*side, groups*C) in the storage type; w[blk] = (w1, w2, w3) in the storage type; gn[blk] = (g1, b1, g2, b2, g3, b3) float32;
    eps[blk] = (eps1, eps2, eps3)"""

    def __init__(self, side, prec, B, groups, nblocks, x, w, gn, eps, note=None):
        self.side, self.prec, self.B, self.groups, self.nblocks = side, prec, B, groups, nblocks
        self.C, self.CM = SHAPES[side]
        self.x, self.w, self.gn, self.eps, self.note = x, w, gn, eps, note or {}

    def trunk(self, g):
        """trunk g alone: its slice of x and of every parameter, as a groups = 1 run"""
        C, CM = self.C, self.CM
        w = [tuple(t[g:g + 1].contiguous() for t in blk) for blk in self.w]
        gn = [tuple(t[g * ch:(g + 1) * ch].contiguous() for t, ch in zip(blk, (CM, CM, CM, CM, C, C))) for blk in self.gn]
        return Run(self.side, self.prec, self.B, 1, self.nblocks, self.x[:, :, g * C:(g + 1) * C].contiguous(), w, gn, self.eps)


def _uniform(gen, *shape):
    return torch.rand(*shape, generator=gen) * 2 - 1


@functools.lru_cache(maxsize=None)
def make_run(side, prec, B, groups, nblocks, seed=0, low_variance=(), offset_ratio=None):
    """low_variance: the convs (0..2) whose weights are multiplied by 2^-8 in every block -- their group variances fall below eps, so eps decides
    the result ((0,): conv1 alone; (0, 1, 2): every GroupNorm of the block is eps-dominated).
    offset_ratio: the construction of tests/test_norm_conditioning_gpu.py's _offset_conv on block 0's conv1 -- the last input channel of every
    trunk is the constant 1, the last weight column carries m = ratio x the standard deviation of the conv without it: conv1's output is
    (noise conv) + m exactly, group |mean| / std about the ratio (note['m'])."""
    C, CM = SHAPES[side]
    tdt = TDT[prec]
    gen = torch.Generator().manual_seed(1000 * seed + 100 * side + 10 * B + groups)
    x = torch.rand(B, side * side, groups * C, generator=gen)
    w, gn, eps = [], [], []
    for blk in range(nblocks):
        w1 = _uniform(gen, groups, CM, C) * (2.0 / C) ** 0.5
        w2 = _uniform(gen, groups, CM, 9 * CM) * (2.0 / (9 * CM)) ** 0.5
        w3 = _uniform(gen, groups, C, CM) * (2.0 / CM) ** 0.5
        w1, w2, w3 = (t * 2.0 ** -8 if i in low_variance else t for i, t in enumerate((w1, w2, w3)))
        w.append([w1.to(tdt), w2.to(tdt), w3.to(tdt)])
        gn.append(tuple(t for ch in (CM, CM, C) for t in (_uniform(gen, groups * ch) * 0.5 + 1.0, _uniform(gen, groups * ch) * 0.1)))
        eps.append(tuple(eps_of(blk, i) for i in range(3)))
    x = x.to(tdt)
    note = {}
    if offset_ratio is not None:
        xv = x.view(B, side * side, groups, C)
        xv[..., -1] = 1.0
        w[0][0][..., -1] = 0.0
        conv = torch.einsum("bpgc,gmc->bpgm", xv.double(), w[0][0].double())
        m = torch.tensor(offset_ratio * conv.std().item()).to(tdt)
        w[0][0][..., -1] = m
        note["m"] = m.item()
    return Run(side, prec, B, groups, nblocks, x, [tuple(b) for b in w], gn, eps, note)


def conv1_out(x, w1, side, dtype=torch.float64):
    """conv1 of one trunk: x (B, side*side, C), w1 [CM][C] -> (B, CM, side, side)"""
    B, C = x.shape[0], x.shape[2]
    xn = x.to(dtype).view(B, side, side, C).permute(0, 3, 1, 2)
    return F.conv2d(xn, w1.to(dtype).view(w1.shape[0], C, 1, 1))


def group_variance(t):
    """biased variance per (sample, GroupNorm group) of an NCHW tensor"""
    return t.reshape(t.shape[0], GN_GROUPS, -1).var(-1, unbiased=False)


def block_ref(x, w, gn, eps, tdt, dtype=torch.float64, variances=None):
    """One identity bottleneck on every trunk of x (B, side*side, groups*C) in `dtype` arithmetic (float64: the reference; float32: the CPU
    restatement the bounds of tests/test_depth_runs_gpu.py were taken from).  tdt: the storage type, rounded to where the kernels store -- the two
    mid tensors and the block output -- or None for no rounding.  w = (w1, w2, w3), gn = (g1, b1, g2, b2, g3, b3), eps = (eps1, eps2, eps3) of this
    block.  Returns (B, side*side, groups*C) in `dtype` (holding storage-type values when tdt is given).  variances: a list of three numbers that
    takes the largest group variance of each conv's output over samples and trunks."""
    w1, w2, w3 = w
    groups, CM, C = w1.shape
    B, HW = x.shape[0], x.shape[1]
    side = int(round(HW ** 0.5))
    rnd = (lambda t: t.to(tdt).to(dtype)) if tdt is not None else (lambda t: t)
    out = torch.empty(B, HW, groups * C, dtype=dtype)
    for g in range(groups):
        p = [t.to(dtype)[g * ch:(g + 1) * ch] for t, ch in zip(gn, (CM, CM, CM, CM, C, C))]
        xin = x[:, :, g * C:(g + 1) * C].to(dtype).reshape(B, side, side, C).permute(0, 3, 1, 2)
        k1 = w1[g].to(dtype).view(CM, C, 1, 1)
        k2 = w2[g].to(dtype).view(CM, 3, 3, CM).permute(0, 3, 1, 2)          # k = (kh*3 + kw)*CM + ci -> OIHW
        k3 = w3[g].to(dtype).view(C, CM, 1, 1)
        c1 = F.conv2d(xin, k1)
        o = rnd(F.relu(F.group_norm(c1, GN_GROUPS, p[0], p[1], eps[0])))
        c2 = F.conv2d(o, k2, padding=1)
        o = rnd(F.relu(F.group_norm(c2, GN_GROUPS, p[2], p[3], eps[1])))
        c3 = F.conv2d(o, k3)
        o = F.group_norm(c3, GN_GROUPS, p[4], p[5], eps[2])
        out[:, :, g * C:(g + 1) * C] = rnd(F.relu(o + xin)).permute(0, 2, 3, 1).reshape(B, HW, C)
        if variances is not None:
            for i, c in enumerate((c1, c2, c3)):
                variances[i] = max(variances[i], group_variance(c).max().item())
    return out


def tolerance_stats(got, ref, tol):
    """(worst |got - ref| / max(1, |ref|) over tol, share of elements that differ at all) -- the two elementwise conditions of the parity tests"""
    got, ref = got.double(), ref.double()
    d = (got - ref).abs()
    return (d / ref.abs().clamp(min=1.0)).max().item() / tol, (d != 0).double().mean().item()
