"""The step's small kernels (csrc/elementwise.hip) through their hcm_op_* entries against the float64 references of tests/step_ops_cases.py.

Every output buffer is pre-filled with NaN (a sentinel for integers) and allocated inside a guard margin of the same fill; Out.check asserts
that no bit outside the logical region changed -- the margins and the columns between the logical width and the row stride.  Input pad columns
hold NaN, so a kernel that reads past its width shows up in its result.

Bounds (none taken from the kernels):
    integer outputs, copies, single products                exact
    f32 outputs                                             1e-5 of the reference tensor's largest element (the training-op suites' bound)
    mean_rows into f32                                      (S + 2) 2^-24 max |x|: an f32 sum of S terms and one division, worst case
    16-bit outputs                                          one ulp of the storage type at the float64 value, not below its subnormal spacing
Each comparison prints `STEPOPS | kernel | case | figure | bound` before it asserts; profiles/step_ops_parity.md holds the figures."""
import ctypes as C

import pytest
import torch

from tests import step_ops_cases as sc

pytestmark = pytest.mark.gpu

ERR_ARG = -1
GUARD = 64              # elements on either side of every output
SENT = -77              # integer outputs
NAN = float("nan")
PRECS = ("fp32", "fp16", "bf16")


def _lib():
    from robo_vln_amd import _lib
    return _lib.lib(), _lib


def _bits(t):
    t = t.contiguous()
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _dev(t, dtype=None):
    return None if t is None else t.to("cuda", dtype if dtype is not None else t.dtype).contiguous()


def _ptr(t, offset=0):
    return None if t is None else C.c_void_p(t.data_ptr() + offset * t.element_size())


def _padded(t, pad, dtype=None):
    """t (..., C) on the device with `pad` trailing NaN columns per row: what a kernel may not read"""
    d = torch.full(t.shape[:-1] + (t.shape[-1] + pad,), NAN, dtype=dtype or t.dtype, device="cuda")
    d[..., :t.shape[-1]] = t.to("cuda", dtype or t.dtype)
    return d


def _report(kernel, case, err, bound):
    print(f"STEPOPS | {kernel} | {case} | {err:.3e} | {bound:.3e}")


class Out:
    """[rows][ld] output inside guard margins, pre-filled; the logical region is columns [col0, col0 + cols) of `rows_sel` (default: all rows)"""

    def __init__(self, rows, ld, dtype=torch.float32, col0=0, cols=None, rows_sel=None):
        self.fp = dtype.is_floating_point
        self.flat = torch.full((2 * GUARD + rows * ld,), NAN if self.fp else SENT, dtype=dtype, device="cuda")
        self.t = self.flat[GUARD:GUARD + rows * ld].view(rows, ld)
        self.col0, self.cols = col0, ld - col0 if cols is None else cols
        self.rows_sel = list(range(rows)) if rows_sel is None else list(rows_sel)
        keep = torch.ones(2 * GUARD + rows * ld, dtype=torch.bool, device="cuda")
        body = keep[GUARD:GUARD + rows * ld].view(rows, ld)
        body[self.rows_sel, self.col0:self.col0 + self.cols] = False
        self.keep = keep
        self.before = _bits(self.flat).clone()

    def ptr(self, col=0):
        return _ptr(self.t, col)

    def logical(self):
        return self.t[self.rows_sel, self.col0:self.col0 + self.cols]

    def check(self, written=True):
        """nothing outside the logical region changed; written: every logical element was stored (and none is NaN)"""
        torch.cuda.synchronize()
        assert torch.equal(_bits(self.flat)[self.keep], self.before[self.keep]), "the launch wrote outside its logical region"
        got = self.logical()
        if written:
            assert not bool((torch.isnan(got) if self.fp else got == SENT).any()), "the launch left output elements unwritten (or produced NaN)"
        return got.cpu()

    def untouched(self):
        torch.cuda.synchronize()
        return torch.equal(_bits(self.flat), self.before)


def _f32_check(kernel, case, got, ref):
    err, bound = (got.double() - ref).abs().max().item(), sc.f32_bound(ref)
    _report(kernel, case, err, bound)
    assert err <= bound, (kernel, case, err, bound)


def _ulp_check(kernel, case, got, ref, prec):
    worst = ((got.double() - ref).abs() / sc.ulp(ref, prec)).max().item()
    _report(kernel, f"{case} [{prec}, ulps]", worst, 1.0)
    assert worst <= 1.0, (kernel, case, prec, worst)


def _storage_check(kernel, case, got, ref, prec):
    (_f32_check(kernel, f"{case} [fp32]", got, ref) if prec == "fp32" else _ulp_check(kernel, case, got, ref, prec))


# ================================================================================================ cells and heads
class Heads:
    """hcm_op_heads over fresh outputs for `rows` states: the weights of a Cell (or given ones), the output buffers and the struct"""

    def __init__(self, rows, H, r, w, b, pred=False, emb=None, emb_rows=sc.EMB_ROWS):
        _, L = _lib()
        self.r, self.pred = r, pred
        self.w, self.b = [_dev(t) for t in w], [_dev(t) for t in b]
        self.out = [Out(rows, sc.head_ld(n), cols=n) if n else None for n in r]
        self.s = L.HcmOpHeadsStruct()
        for i, n in enumerate(r):
            if n:
                setattr(self.s, f"w{i}", self.w[i].data_ptr()); setattr(self.s, f"b{i}", self.b[i].data_ptr())
                setattr(self.s, f"out{i}", self.out[i].t.data_ptr()); setattr(self.s, f"r{i}", n); setattr(self.s, f"ld{i}", sc.head_ld(n))
        self.pred_out = self.emb_out = None
        if pred:
            self.emb = _dev(emb)
            self.pred_out, self.emb_out = Out(rows, 1, torch.int64), Out(rows, sc.EMB_LD, cols=emb.shape[1])
            self.s.pred, self.s.emb, self.s.emb_out = self.pred_out.t.data_ptr(), self.emb.data_ptr(), self.emb_out.t.data_ptr()
            self.s.emb_rows, self.s.emb_dim, self.s.emb_ld = emb_rows, emb.shape[1], sc.EMB_LD

    def ref(self):
        return C.byref(self.s)

    def collect(self, written=True):
        res = {f"out{i}": o.check(written) for i, o in enumerate(self.out) if o is not None}
        if self.pred:
            res["pred"], res["emb_out"] = self.pred_out.check()[:, 0], self.emb_out.check(written)
        return res


XH_COL0, XH_PAD = 3, 5


def run_cell(c, alias=False, bad0=None, heads=True, rc_want=0):
    """one hcm_op_rnn_cell launch on Cell c; returns every output on the host.  alias: h_out is h_in's own buffer"""
    lib, _ = _lib()
    gates, gh, mask = _dev(c.gates), _dev(c.gh), _dev(c.mask)
    h_in = _dev(c.h_in)
    h_out = None if alias else Out(c.R * c.B, c.H)
    xh = Out(c.B, XH_COL0 + c.H + XH_PAD, col0=XH_COL0, cols=c.H)
    hd = Heads(c.B, c.H, c.r, c.w, c.b, c.pred, c.emb) if heads else None
    bad = torch.tensor([bad0], dtype=torch.int32, device="cuda") if bad0 is not None else None
    rc = lib.hcm_op_rnn_cell(_ptr(gates), _ptr(gh), _ptr(h_in), _ptr(mask), _ptr(h_in) if alias else h_out.ptr(), xh.ptr(), xh.t.shape[1], XH_COL0,
                             hd.ref() if hd else None, _ptr(bad), c.B, c.H, c.kind, None)
    assert rc == rc_want, rc
    torch.cuda.synchronize()
    if rc_want:
        assert (alias or h_out.untouched()) and xh.untouched() and all(o is None or o.untouched() for o in (hd.out if hd else []))
        return None
    res = hd.collect(written=False) if hd else {}
    res["h_out"] = (h_in.cpu() if alias else h_out.check(written=False)).view(c.R, c.B, c.H)
    res["xh"] = xh.check(written=False)
    if not alias:
        assert torch.equal(_bits(h_in.cpu()), _bits(c.h_in)), "the launch changed h_in"
    if bad is not None:
        res["bad"] = int(bad.item())
    return res


def _same(a, b, keys=None):
    for k in keys or a:
        if not torch.equal(_bits(a[k]) if torch.is_tensor(a[k]) else torch.tensor(a[k]), _bits(b[k]) if torch.is_tensor(b[k]) else torch.tensor(b[k])):
            return k
    return None


@pytest.mark.parametrize("headset", list(sc.HEADSETS))
@pytest.mark.parametrize("H", sc.CELL_H)
@pytest.mark.parametrize("kind", [sc.LSTM, sc.GRU], ids=["lstm", "gru"])
def test_rnn_cell_matches_single_forward(kind, H, headset):
    """B = 5 with masks 1 0 1 1 0 against float64; the fused heads, argmax and embedding row; rnn_prep's product; a stale state behind a zero
    mask ignored exactly; h_out aliasing h_in; two runs; every sample alone (B = 1) with the bits it has inside the batch"""
    c = sc.Cell(kind, H, headset)
    got = run_cell(c)
    case = f"{'lstm' if kind == sc.LSTM else 'gru'} H{H} {headset}"
    ref = sc.cell_ref(kind, c.gates, c.gh, c.h_in, c.mask)
    assert not bool(torch.isnan(got["h_out"]).any())
    for i, name in enumerate(("h", "c")[:c.R]):
        _f32_check("rnn_cell " + name, case, got["h_out"][i], ref[i])
    assert torch.equal(_bits(got["xh"]), _bits(sc.rnn_prep_ref(c.h_in, c.mask))), "rnn_prep: one product, exact"
    hr = sc.heads_ref(ref[0], c.w, c.b)
    for i, n in enumerate(c.r):
        if n:
            _f32_check(f"rnn_cell head{i}", case, got[f"out{i}"], hr[i])
    if c.pred:
        want = torch.argmax(got["out0"], dim=1)                 # torch.argmax on the very logits the record holds
        assert torch.equal(got["pred"], want)
        top = hr[0].topk(2, dim=1).values
        clear = (top[:, 0] - top[:, 1]) > 10 * sc.f32_bound(hr[0])
        assert bool(clear.any()) and torch.equal(got["pred"][clear], torch.argmax(hr[0], dim=1)[clear])      # ... and on the float64 logits where they decide
        if c.r[0] > sc.EMB_ROWS:
            assert bool((want >= sc.EMB_ROWS).any()), "no winner beyond the embedding table: the clamp is not exercised"
        assert torch.equal(_bits(got["emb_out"]), _bits(c.emb[want.clamp_max(sc.EMB_ROWS - 1)]))
    # a masked sample's stale state is ignored exactly: zeroing it changes no bit
    z = sc.Cell(kind, H, headset)
    z.h_in[:, z.mask == 0] = 0.0
    got_z = run_cell(z)
    assert _same(got, got_z, [k for k in got if k != "xh"]) is None
    assert bool((got["xh"][c.mask == 0] == 0).all())
    assert _same(got, run_cell(c)) is None, "two runs differ"
    al = run_cell(c, alias=True)
    assert _same(got, al) is None, "h_out aliasing h_in changes the result"
    for b in range(c.B):
        one = run_cell(c.row(b))
        for k in got:
            full = got[k][:, b:b + 1] if k == "h_out" else got[k][b:b + 1]
            assert torch.equal(_bits(one[k]), _bits(full)), (k, b)


@pytest.mark.parametrize("kind", [sc.LSTM, sc.GRU], ids=["lstm", "gru"])
def test_rnn_cell_guard_counts_poisoned_samples_once(kind):
    """+inf in one gate of sample 1 and NaN in another of sample 3: the counter rises by exactly 2 from its pre-loaded value, and every other
    sample keeps the bits of the clean call"""
    c = sc.Cell(kind, 96, "r2_1_tanh")
    clean = run_cell(c, bad0=10)
    assert clean["bad"] == 10
    p = sc.Cell(kind, 96, "r2_1_tanh")
    p.gates[1, 2 * 96 + 5] = float("inf")
    p.gates[1, 7] = float("inf")                       # a second one in the same sample: still one count
    (p.gh if kind == sc.GRU else p.gates)[3, 95] = NAN
    got = run_cell(p, bad0=10)
    assert got["bad"] == 12
    for b in (0, 2, 4):
        for k in ("out0", "out1", "out2", "xh"):
            assert torch.equal(_bits(got[k][b]), _bits(clean[k][b])), (k, b)
        assert torch.equal(_bits(got["h_out"][:, b]), _bits(clean["h_out"][:, b])), b
    assert "bad" not in run_cell(c)                     # the counter is optional


@pytest.mark.parametrize("kind", [sc.LSTM, sc.GRU], ids=["lstm", "gru"])
def test_rnn_cell_refuses_a_fused_pred_beyond_64_logits(kind):
    """heads_eval keeps the fused argmax's logits in 64 words of LDS: r0 = 65 with pred is HCM_ERR_ARG without a launch (r0 = 64 runs:
    test_rnn_cell_matches_single_forward), and without pred 65 rows are fine"""
    c = sc.Cell(kind, 96, "r4_pred")
    c.r, c.w, c.b = (65, 0, 0), [sc.uni(sc.gen(1), 65, 96), c.w[1], c.w[2]], [sc.uni(sc.gen(2), 65), c.b[1], c.b[2]]
    run_cell(c, rc_want=ERR_ARG)
    c.pred = False
    got = run_cell(c)
    _f32_check("rnn_cell head0", f"kind {kind} r0 65 without pred", got["out0"], sc.heads_ref(sc.cell_ref(kind, c.gates, c.gh, c.h_in, c.mask)[0], c.w, c.b)[0])
    # bad arguments of the entry itself
    lib, _ = _lib()
    t = torch.zeros(4 * 96 * 5, device="cuda")
    assert lib.hcm_op_rnn_cell(_ptr(t), None if kind == sc.GRU else _ptr(t), _ptr(t), _ptr(t), _ptr(t), None, 0, 0, None, None, 5, 96, kind, None) == ERR_ARG
    assert lib.hcm_op_rnn_cell(_ptr(t), _ptr(t) if kind == sc.GRU else None, _ptr(t), _ptr(t), _ptr(t), None, 0, 0, None, None, 0, 96, kind, None) == ERR_ARG
    assert lib.hcm_op_rnn_cell(_ptr(t), _ptr(t) if kind == sc.GRU else None, _ptr(t), _ptr(t), _ptr(t), None, 0, 0, None, None, 5, 96, 2, None) == ERR_ARG


@pytest.mark.parametrize("headset", list(sc.HEADSETS))
@pytest.mark.parametrize("rows", [1, 7])
@pytest.mark.parametrize("H", sc.CELL_H)
def test_heads_rows_matches_float64_and_the_cells_heads(rows, H, headset):
    """the same head sets (without the fused pred, which heads_rows refuses) over `rows` states: against float64, and bit-equal to what
    hcm_op_rnn_cell's fused heads give for the same hidden rows"""
    lib, _ = _lib()
    c = sc.Cell(sc.GRU, H, headset, B=rows, seed=2)
    c.pred = False
    cell = run_cell(c)
    hs = cell["h_out"][0]
    hd = Heads(rows, H, c.r, c.w, c.b)
    hsd = _dev(hs)
    assert lib.hcm_op_heads_rows(_ptr(hsd), hd.ref(), rows, H, None) == 0
    got = hd.collect()
    ref = sc.heads_ref(hs, c.w, c.b)
    for i, n in enumerate(c.r):
        if n:
            _f32_check(f"heads_rows head{i}", f"rows {rows} H{H} {headset}", got[f"out{i}"], ref[i])
            assert torch.equal(_bits(got[f"out{i}"]), _bits(cell[f"out{i}"])), i
    hd2 = Heads(rows, H, c.r, c.w, c.b)
    assert lib.hcm_op_heads_rows(_ptr(hsd), hd2.ref(), rows, H, None) == 0
    assert _same(got, hd2.collect()) is None
    for b in range(rows):
        one = Heads(1, H, c.r, c.w, c.b)
        assert lib.hcm_op_heads_rows(_ptr(hsd, b * H), one.ref(), 1, H, None) == 0
        for k, v in one.collect().items():
            assert torch.equal(_bits(v), _bits(got[k][b:b + 1])), (k, b)
    if c.r[0] >= 1:
        bad = Heads(rows, H, c.r, c.w, c.b, True, c.emb)
        assert lib.hcm_op_heads_rows(_ptr(hsd), bad.ref(), rows, H, None) == ERR_ARG
        assert all(o is None or o.untouched() for o in bad.out) and bad.pred_out.untouched()
    assert lib.hcm_op_heads_rows(_ptr(hsd), hd.ref(), 0, H, None) == ERR_ARG


# ================================================================================================ argmax, stand-alone and fused
def _argmax_fused(rows):
    """the rows pushed through hcm_op_rnn_cell's fused pred: a GRU step that passes its (finite) state through exactly -- z = sigmoid(100) = 1,
    n = tanh(0) = 0 -- and a head that rebuilds the row from it: logit r = 2^100 (s[r] + s[n + r] + s[2n + r]) with s[r] = row[r] 2^-100 for a
    finite entry, +-2^30 for an infinite one (the product overflows), and s[n + r] = 2^30, s[2n + r] = -2^30 for a NaN (inf - inf)"""
    lib, _ = _lib()
    B, n = rows.shape
    H = 3 * n
    s = torch.zeros(B, H)
    fin = torch.isfinite(rows)
    s[:, :n] = torch.where(fin, rows * 2.0 ** -100, torch.zeros_like(rows))
    s[:, :n] += torch.where(torch.isinf(rows), torch.sign(rows) * 2.0 ** 30, torch.zeros_like(rows))
    s[:, n:2 * n] = torch.where(torch.isnan(rows), torch.full_like(rows, 2.0 ** 30), torch.zeros_like(rows))
    s[:, 2 * n:] = torch.where(torch.isnan(rows), torch.full_like(rows, -(2.0 ** 30)), torch.zeros_like(rows))      # (no -0.0: the step returns +0 for it)
    w0 = torch.cat([torch.eye(n)] * 3, dim=1) * 2.0 ** 100
    c = sc.Cell(sc.GRU, H, "r4_pred", B=B)
    c.gates, c.gh = torch.zeros(B, 3 * H), torch.zeros(B, 3 * H)
    c.gates[:, H:2 * H] = 100.0
    c.h_in, c.mask = s[None].clone(), torch.ones(B)
    c.r, c.w, c.b = (n, 0, 0), [w0, c.w[1], c.w[2]], [torch.zeros(n), c.b[1], c.b[2]]
    c.emb = sc.uni(sc.gen(9), n, sc.EMB_DIM)
    lib_heads = Heads(B, H, c.r, c.w, c.b, True, c.emb, emb_rows=n)
    gates, gh, mask, h_in = _dev(c.gates), _dev(c.gh), _dev(c.mask), _dev(c.h_in)
    h_out = Out(B, H)
    assert lib.hcm_op_rnn_cell(_ptr(gates), _ptr(gh), _ptr(h_in), _ptr(mask), h_out.ptr(), None, 0, 0, lib_heads.ref(), None, B, H, sc.GRU, None) == 0
    assert torch.equal(_bits(h_out.check()), _bits(s)), "the pass-through step changed the state"
    return lib_heads.collect(written=False), c.emb


@pytest.mark.parametrize("n", sc.ARGMAX_N)
def test_argmax_is_torch_argmax_at_both_sites(n):
    """70 rows (two workgroups of the stand-alone kernel) of n logits at stride 7, pad columns NaN: exact ties at every pair of positions,
    all-equal, -inf, +inf, a NaN at index 0 and above it.  hcm_op_argmax and the fused pred of hcm_op_rnn_cell must both give torch.argmax"""
    lib, _ = _lib()
    rows = sc.argmax_rows(n)
    want = torch.argmax(rows, dim=1)
    x = _padded(rows, sc.ARGMAX_LD - n)
    pred = Out(sc.ARGMAX_B, 1, torch.int64)
    assert lib.hcm_op_argmax(_ptr(x), pred.ptr(), sc.ARGMAX_B, n, sc.ARGMAX_LD, None) == 0
    alone = pred.check()[:, 0]
    wrong = torch.nonzero(alone != want).flatten().tolist()
    assert not wrong, f"hcm_op_argmax differs from torch.argmax on rows {[(r, rows[r].tolist(), int(alone[r]), int(want[r])) for r in wrong[:4]]}"
    again = Out(sc.ARGMAX_B, 1, torch.int64)
    assert lib.hcm_op_argmax(_ptr(x), again.ptr(), sc.ARGMAX_B, n, sc.ARGMAX_LD, None) == 0 and torch.equal(again.check()[:, 0], alone)
    fused, emb = _argmax_fused(rows)
    logits = fused["out0"]
    assert torch.equal(torch.isnan(logits), torch.isnan(rows)) and torch.equal(logits.nan_to_num(nan=0.0), rows.nan_to_num(nan=0.0)), "the head did not rebuild the rows"
    wrong = torch.nonzero(fused["pred"] != want).flatten().tolist()
    assert not wrong, f"the fused pred differs from torch.argmax on rows {[(r, rows[r].tolist(), int(fused['pred'][r]), int(want[r])) for r in wrong[:4]]}"
    assert torch.equal(fused["pred"], alone)
    assert torch.equal(_bits(fused["emb_out"]), _bits(emb[want]))
    assert lib.hcm_op_argmax(_ptr(x), pred.ptr(), sc.ARGMAX_B, 8, sc.ARGMAX_LD, None) == ERR_ARG        # n > ld


# ================================================================================================ one-query attention
def _attn_launch(q, k, v, lens, scale, inter, b0=0, B=None):
    """samples b0 .. b0 + B - 1; inputs on padded strides (pad columns NaN), or k | v interleaved in one buffer"""
    lib, _ = _lib()
    Bq, S, D, Dv = q.shape[0], k.shape[1], q.shape[1], v.shape[2]
    B = Bq if B is None else B
    qd = _padded(q, 3)
    if inter:
        kv = _dev(torch.cat([k, v], dim=2))
        kp, vp, ldk, ldv = _ptr(kv, b0 * S * (D + Dv)), _ptr(kv, b0 * S * (D + Dv) + D), D + Dv, D + Dv
    else:
        kd, vd = _padded(k, 2), _padded(v, 4)
        kp, vp, ldk, ldv = _ptr(kd, b0 * S * (D + 2)), _ptr(vd, b0 * S * (Dv + 4)), D + 2, Dv + 4
    ld = _dev(lens)
    out = Out(B, Dv + 5, cols=Dv)
    assert lib.hcm_op_attn1q(_ptr(qd, b0 * (D + 3)), D + 3, kp, ldk, vp, ldv, _ptr(ld, b0) if ld is not None else None, out.ptr(), Dv + 5, B, S, D, Dv,
                             scale, None) == 0
    return out.check()


@pytest.mark.parametrize("case", sc.ATTN_CASES, ids=sc.attn_id)
def test_attn1q_matches_cma_attn(case):
    q, k, v, lens, scale = sc.make_attn(case)
    got = _attn_launch(q, k, v, lens, scale, case[4])
    _f32_check("attn1q", sc.attn_id(case), got, sc.attn_ref(q, k, v, lens, scale))
    assert torch.equal(_bits(got), _bits(_attn_launch(q, k, v, lens, scale, case[4])))
    for b in range(q.shape[0]):
        assert torch.equal(_bits(_attn_launch(q, k, v, lens, scale, case[4], b, 1)), _bits(got[b:b + 1])), b
    lib, _ = _lib()
    t = torch.zeros(64, device="cuda")
    assert lib.hcm_op_attn1q(_ptr(t), 8, _ptr(t), 4, _ptr(t), 8, None, _ptr(t), 8, 1, 1, 8, 8, 1.0, None) == ERR_ARG       # ldk < D
    assert lib.hcm_op_attn1q(_ptr(t), 8, _ptr(t), 8, _ptr(t), 8, None, _ptr(t), 8, 1, 0, 8, 8, 1.0, None) == ERR_ARG       # S = 0


# ================================================================================================ pools
def _pool_launch(xd, B, H, W, C, OH, OW, prec, ldx=None, off=0):
    lib, _ = _lib()
    y = Out(B * OH * OW, C + 8, sc.TDT[prec], cols=C)
    assert lib.hcm_op_adaptive_avgpool(_ptr(xd, off), y.ptr(), sc.CODE[prec], B, H, W, C, OH, OW, ldx or C, C + 8, None) == 0
    return y.check().view(B, OH, OW, C)


@pytest.mark.parametrize("case", sc.POOL_CASES, ids=lambda c: "%dx%d_to_%dx%d" % c)
@pytest.mark.parametrize("prec", PRECS)
def test_adaptive_avgpool_matches_torch(prec, case):
    H, W, OH, OW = case
    B, C = sc.POOL_B, sc.POOL_C
    xs, x64 = sc.make_pool_input(B, H, W, C, prec)
    xd = _dev(xs)
    got = _pool_launch(xd, B, H, W, C, OH, OW, prec)
    _storage_check("adaptive_avgpool", "%dx%d->%dx%d" % case, got, sc.adaptive_pool_ref(x64, OH, OW), prec)
    if (H, W) == (OH, OW):
        assert torch.equal(_bits(got), _bits(xs)), "same-size pooling must be an exact copy"
    if (H, W, OH, OW) == (2, 2, 4, 4):
        assert torch.equal(_bits(got), _bits(xs.repeat_interleave(2, 1).repeat_interleave(2, 2))), "windows of one element must copy it"
    assert torch.equal(_bits(got), _bits(_pool_launch(xd, B, H, W, C, OH, OW, prec)))
    for b in range(B):
        assert torch.equal(_bits(_pool_launch(xd, 1, H, W, C, OH, OW, prec, off=b * H * W * C)[0]), _bits(got[b])), b


@pytest.mark.parametrize("prec", PRECS)
def test_adaptive_avgpool_on_one_half_of_a_channel_pair(prec):
    """the hi | lo form: ldx = 2C with a channel-offset base pointer, ldy > C -- either half must carry the bits of the dense launch on it"""
    B, C, (H, W, OH, OW) = sc.POOL_B, sc.POOL_C, (5, 7, 4, 4)
    xs, x64 = sc.make_pool_input(B, H, W, 2 * C, prec, seed=5)
    xd = _dev(xs)
    for half in (0, 1):
        got = _pool_launch(xd, B, H, W, C, OH, OW, prec, ldx=2 * C, off=half * C)
        dense = _pool_launch(_dev(xs[..., half * C:(half + 1) * C]), B, H, W, C, OH, OW, prec)
        assert torch.equal(_bits(got), _bits(dense)), half
        _storage_check("adaptive_avgpool", f"5x7->4x4 half {half} of ldx 2C", got, sc.adaptive_pool_ref(x64[..., half * C:(half + 1) * C], OH, OW), prec)
    lib, _ = _lib()
    y = Out(B * 16, C + 8, sc.TDT[prec], cols=C)
    assert lib.hcm_op_adaptive_avgpool(_ptr(xd), y.ptr(), sc.CODE[prec], B, H, W, C + 2, OH, OW, 2 * C, C + 8, None) == ERR_ARG and y.untouched()
    assert lib.hcm_op_adaptive_avgpool(_ptr(xd), y.ptr(), sc.CODE[prec], B, H, W, C, OH, OW, C - 8, C + 8, None) == ERR_ARG and y.untouched()


def _mean_launch(xd, lens_d, B, S, C, prec, out_f32, b0=0):
    lib, _ = _lib()
    y = Out(B, C + 16, torch.float32 if out_f32 else sc.TDT[prec], col0=8, cols=C)
    assert lib.hcm_op_mean_rows(_ptr(xd, b0 * S * (C + 8)), y.ptr(8), sc.CODE[prec], B, S, C, C + 8, C + 16, out_f32,
                                _ptr(lens_d, b0) if lens_d is not None else None, None) == 0
    return y.check()


@pytest.mark.parametrize("out_f32", [0, 1])
@pytest.mark.parametrize("case", sc.MEAN_CASES, ids=lambda c: "B%d_S%d_C%d" % c[:3] + ("_lens" if c[3] else ""))
@pytest.mark.parametrize("prec", PRECS)
def test_mean_rows_matches_float64(prec, case, out_f32):
    """lens [37, 5, 0, 100] at S = 37: the clamp to [1, S] include/hcm.h states; rows beyond a sample's length hold NaN and must not be read"""
    B, S, C, lens = case
    g = sc.gen(S + C)
    x = sc.uni(g, B, S, C, lo=(0.0 if prec != "fp32" else -1.0), hi=1.0)        # 16-bit: a ReLU feature map, as the trunk's token mean reads
    xs, x64 = sc.stored(x, prec)
    xd = _padded(xs, 8)
    if lens:
        for b, l in enumerate(lens):
            xd[b, min(max(l, 1), S):] = NAN
    lens_d = _dev(torch.tensor(lens, dtype=torch.int32)) if lens else None
    got = _mean_launch(xd, lens_d, B, S, C, prec, out_f32)
    ref = sc.mean_rows_ref(x64, lens)
    name = "B%d S%d C%d" % case[:3] + (" lens" if lens else "")
    if out_f32 or prec == "fp32":
        err, bound = (got.double() - ref).abs().max().item(), (S + 2) * 2.0 ** -24 * x64.abs().max().item()
        _report("mean_rows", f"{name} [{prec} -> f32]", err, bound)
        assert err <= bound, (err, bound)
    else:
        _ulp_check("mean_rows", name, got, ref, prec)
    assert torch.equal(_bits(got), _bits(_mean_launch(xd, lens_d, B, S, C, prec, out_f32)))
    for b in range(B):
        assert torch.equal(_bits(_mean_launch(xd, lens_d, 1, S, C, prec, out_f32, b)), _bits(got[b:b + 1])), b


@pytest.mark.parametrize("case", sc.AVGPOOL2_CASES, ids=lambda c: "B%d_%dx%d" % c)
@pytest.mark.parametrize("prec", PRECS)
def test_avgpool2_matches_torch_and_its_padded_form(prec, case):
    lib, _ = _lib()
    B, H, W = case
    x = sc.uni(sc.gen(H * W), B, H, W, lo=0.0, hi=1.0)              # a depth frame
    xd = _dev(x)
    Ho, Wo = H // 2, W // 2

    def plain(xp, Bn):
        y = Out(Bn * Ho, Wo, sc.TDT[prec])
        assert lib.hcm_op_avgpool2(xp, y.ptr(), sc.CODE[prec], Bn, H, W, 0, None) == 0
        return y.check().view(Bn, Ho, Wo)
    got = plain(_ptr(xd), B)
    _storage_check("avgpool2", "B%d %dx%d" % case, got, sc.avgpool2_ref(x), prec)
    assert torch.equal(_bits(got), _bits(plain(_ptr(xd), B)))
    for b in range(B):
        assert torch.equal(_bits(plain(_ptr(xd, b * H * W), 1)[0]), _bits(got[b])), b
    yp = Out(B * (Ho + 6), Wo + 8, sc.TDT[prec])
    rc = lib.hcm_op_avgpool2(_ptr(xd), yp.ptr(), sc.CODE[prec], B, H, W, 1, None)
    if prec == "fp32":
        assert rc == ERR_ARG and yp.untouched()                     # the packed stem frame exists in the 16-bit types only
        return
    assert rc == 0
    pad = yp.check().view(B, Ho + 6, Wo + 8)
    assert torch.equal(_bits(pad[:, 3:3 + Ho, 3:3 + Wo]), _bits(got)), "the padded form's interior must carry the plain form's bits"
    border = pad.clone()
    border[:, 3:3 + Ho, 3:3 + Wo] = 0
    assert bool((_bits(border) == 0).all()), "the border must be exact (positive) zeros"
    assert lib.hcm_op_avgpool2(_ptr(xd), yp.ptr(), sc.CODE[prec], B, H, W - 1, 0, None) == ERR_ARG


# ================================================================================================ embedding front ends
def _bert_launch(ids, idt, t, prec, D):
    lib, _ = _lib()
    code, tdt = sc.IDS[idt]
    B, L = ids.shape
    idd = _dev(ids.to(tdt))
    td = {k: _dev(v) for k, v in t.items()}
    y = Out(B * L, D, sc.TDT[prec])
    assert lib.hcm_op_bert_embed(_ptr(idd), code, _ptr(td["word"]), _ptr(td["pos"]), _ptr(td["type0"]), _ptr(td["gamma"]), _ptr(td["beta"]), y.ptr(),
                                 sc.CODE[prec], B, L, D, sc.BERT_VOCAB, 1e-12, None) == 0
    return y.check().view(B, L, D)


@pytest.mark.parametrize("D", [768, 64])
@pytest.mark.parametrize("L", [1, 7])
@pytest.mark.parametrize("prec", PRECS)
def test_bert_embed_matches_bert_embeddings(prec, L, D):
    """B L = 2 and 14 rows, no multiple of the four rows a workgroup takes; ids 0, vocab - 1, -3 and vocab + 5: the clamp of include/hcm.h"""
    ids = torch.tensor(sc.BERT_IDS[L])
    t = sc.make_bert_tables(D)
    got = _bert_launch(ids, "i64", t, prec, D)
    _storage_check("bert_embed", f"L{L} D{D}", got, sc.bert_embed_ref(ids, t), prec)
    for idt in ("i32", "f32"):
        assert torch.equal(_bits(_bert_launch(ids, idt, t, prec, D)), _bits(got)), idt
    for b in range(2):
        assert torch.equal(_bits(_bert_launch(ids[b:b + 1], "i64", t, prec, D)), _bits(got[b:b + 1])), b
    lib, _ = _lib()
    z = torch.zeros(8, device="cuda")
    assert lib.hcm_op_bert_embed(_ptr(z), sc.CODE["fp16"], _ptr(z), _ptr(z), _ptr(z), _ptr(z), _ptr(z), _ptr(z), 0, 1, 1, 64, 50, 1e-12, None) == ERR_ARG     # ids as fp16


@pytest.mark.parametrize("L", [1, 9])
def test_instr_embed_matches_the_instruction_encoders_front_end(L):
    """E = 50 into ldx = 64: the pad columns are exact zeros; lengths = the count of non-zero ids, a zero in the middle not counted"""
    lib, _ = _lib()
    ids = torch.tensor(sc.INSTR_IDS[L])
    B = ids.shape[0]
    table = sc.uni(sc.gen(L), sc.INSTR_VOCAB, sc.INSTR_E)
    td = _dev(table)
    res = {}
    for idt, (code, tdt) in sc.IDS.items():
        idd = _dev(ids.to(tdt))
        x, lens = Out(B * L, sc.INSTR_LDX), Out(B, 1, torch.int32)
        assert lib.hcm_op_instr_embed(_ptr(idd), code, _ptr(td), x.ptr(), lens.ptr(), B, L, sc.INSTR_E, sc.INSTR_LDX, sc.INSTR_VOCAB, None) == 0
        res[idt] = (x.check().view(B, L, sc.INSTR_LDX), lens.check()[:, 0])
        assert torch.equal(_bits(res[idt][0]), _bits(sc.instr_embed_ref(ids, table, sc.INSTR_LDX))), idt
        assert bool((_bits(res[idt][0][:, :, sc.INSTR_E:]) == 0).all())
        assert torch.equal(res[idt][1].long(), sc.instr_lengths_ref(ids)), idt
    # ids outside the table: the lookup clamps, the count does not care
    wild = torch.tensor([[-3, 55, 0]])
    x, lens = Out(3, sc.INSTR_LDX), Out(1, 1, torch.int32)
    wd = _dev(wild)
    assert lib.hcm_op_instr_embed(_ptr(wd), sc.IDS["i64"][0], _ptr(td), x.ptr(), lens.ptr(), 1, 3, sc.INSTR_E, sc.INSTR_LDX, sc.INSTR_VOCAB, None) == 0
    assert torch.equal(_bits(x.check().view(1, 3, -1)), _bits(sc.instr_embed_ref(wild, table, sc.INSTR_LDX))) and lens.check().item() == 2
    assert lib.hcm_op_instr_embed(_ptr(wd), sc.IDS["i64"][0], _ptr(td), x.ptr(), lens.ptr(), 1, 3, sc.INSTR_E, sc.INSTR_E - 1, sc.INSTR_VOCAB, None) == ERR_ARG


# ================================================================================================ LayerNorm of the f32 stream
def _ln_launch(xd, gd, bd, prec, rows, D, form, r0=0):
    lib, _ = _lib()
    y16 = Out(rows, D, sc.TDT[prec])
    y32, stats = (Out(rows, D) if form == "y32" else None), (Out(rows, 2) if form == "stats" else None)
    assert lib.hcm_op_layernorm_f32in(_ptr(xd, r0 * D), _ptr(gd), _ptr(bd), y16.ptr(), y32.ptr() if y32 else None, stats.ptr() if stats else None,
                                      sc.CODE[prec], rows, D, 1e-12, None) == 0
    return y16.check(), (y32.check() if y32 else None), (stats.check() if stats else None)


def _ln_case(prec, rows, D, offset):
    x, gamma, beta = sc.make_ln(rows, D, offset)
    xd, gd, bd = _dev(x), _dev(gamma), _dev(beta)
    ref, mean, rstd = sc.layernorm_ref(x, gamma, beta)
    name = f"rows {rows} D{D}" + (f" offset {offset:g}" if offset else "")
    a16, a32, _ = _ln_launch(xd, gd, bd, prec, rows, D, "y32")
    b16, _, st = _ln_launch(xd, gd, bd, prec, rows, D, "stats")
    _f32_check("layernorm_f32in y32", f"{name} [{prec}]", a32, ref)
    _f32_check("layernorm_f32in mean", f"{name} [{prec}]", st[:, 0], mean)
    _f32_check("layernorm_f32in rstd", f"{name} [{prec}]", st[:, 1], rstd)
    twin = ((a16.double() - b16.double()).abs() / torch.maximum(sc.ulp(a16.double(), prec), sc.ulp(b16.double(), prec))).max().item()
    _report("layernorm_f32in y16 of the two forms", f"{name} [{prec}, ulps]", twin, 1.0)
    assert twin <= 1.0
    assert torch.equal(_bits(a16), _bits(_ln_launch(xd, gd, bd, prec, rows, D, "y32")[0]))
    for r in range(0, rows, 5):
        one = _ln_launch(xd, gd, bd, prec, 1, D, "y32", r)
        assert torch.equal(_bits(one[0]), _bits(a16[r:r + 1])) and torch.equal(_bits(one[1]), _bits(a32[r:r + 1])), r
    worst = [((y.double() - ref).abs() / sc.ulp(ref, prec)).max().item() for y in (a16, b16)]
    for form, w in zip(("y32", "stats"), worst):
        _report("layernorm_f32in y16", f"{name} ({form} form) [{prec}, ulps]", w, 1.0)
    assert max(worst) <= 1.0, (name, prec, worst)


@pytest.mark.parametrize("D", sc.LN_D)
@pytest.mark.parametrize("rows", sc.LN_ROWS)
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_layernorm_f32in_matches_float64(prec, rows, D):
    _ln_case(prec, rows, D, 0.0)


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_layernorm_f32in_rows_offset_by_a_hundred_standard_deviations(prec):
    """x = 100 + N(0, 1).  A mean near 100 held in ONE float32 is off by up to half a float32 ulp of 100, 3.8e-6, however it is summed; that
    error passes into every (x - mean) rstd gamma + beta, and an output below 2^-9 in magnitude has an fp16 spacing under it: with the plain
    two-pass form y16 missed its float64 value by 74 ulps in fp16 and 9.6 in bf16.  The kernels now take the mean of the residuals x - mean
    as a correction on rows whose mean lies beyond 4 standard deviations (ln_f32in_offset_fix; rows nearer zero keep their bits)."""
    _ln_case(prec, 7, 768, 100.0)


def test_layernorm_f32in_refusals():
    lib, _ = _lib()
    x = torch.zeros(7, 256, device="cuda")
    y16, y32, st = Out(7, 256, torch.float16), Out(7, 256), Out(7, 2)
    args = (_ptr(x), _ptr(x), _ptr(x), y16.ptr())
    assert lib.hcm_op_layernorm_f32in(*args, y32.ptr(), st.ptr(), sc.CODE["fp16"], 7, 256, 1e-12, None) == ERR_ARG      # both forms at once
    assert lib.hcm_op_layernorm_f32in(*args, None, None, sc.CODE["fp16"], 7, 256, 1e-12, None) == ERR_ARG               # neither
    assert lib.hcm_op_layernorm_f32in(*args, y32.ptr(), None, sc.CODE["fp32"], 7, 256, 1e-12, None) == ERR_ARG          # a 32-bit operand type
    assert lib.hcm_op_layernorm_f32in(*args, y32.ptr(), None, sc.CODE["fp16"], 7, 128, 1e-12, None) == ERR_ARG          # a width without a kernel
    assert y16.untouched() and y32.untouched() and st.untouched()


# ================================================================================================ range check
@pytest.mark.parametrize("poison", [False, True], ids=["finite", "poisoned"])
@pytest.mark.parametrize("case", sc.ABSMAX_CASES, ids=lambda c: "%dx%d_ld%d" % c)
@pytest.mark.parametrize("prec", PRECS)
def test_absmax_is_exact_and_only_grows(prec, case, poison):
    lib, _ = _lib()
    rows, cols, ld = case
    x = sc.make_absmax(rows, cols, ld, prec, poison)
    xd = _dev(x)
    mx, bad = sc.absmax_ref(x, cols)
    as_bits = lambda f: int(torch.tensor(f, dtype=torch.float32).view(torch.int32).item())
    for pre, cnt in ((0.0, 0), (0.5, 7), (3.0e38, 7)):          # a pre-loaded slot: below and above this tensor's maximum
        slot = Out(1, 2, torch.int32)
        slot.t[0, 0], slot.t[0, 1] = as_bits(pre), cnt
        before = slot.t.clone()
        assert lib.hcm_op_absmax(_ptr(xd), sc.CODE[prec], rows, cols, ld, slot.ptr(), None) == 0
        got = slot.check()[0].tolist()
        assert got == [max(as_bits(pre), as_bits(mx)), cnt + bad], (prec, case, pre, got, as_bits(mx), bad)
        assert got[0] >= before[0, 0].item() and got[1] >= before[0, 1].item()


# ================================================================================================ exact glue
def test_embed_rows_clamps_its_index():
    lib, _ = _lib()
    emb = sc.uni(sc.gen(1), 5, 32)
    idx = torch.tensor([0, 4, -2, 7, 2, 1 << 40, -(1 << 40)])
    y = Out(7, 48, col0=9, cols=32)
    ed, idd = _dev(emb), _dev(idx)
    assert lib.hcm_op_embed_rows(_ptr(ed), _ptr(idd), y.ptr(), 7, 32, 48, 9, 5, None) == 0
    assert torch.equal(_bits(y.check()), _bits(emb[idx.clamp(0, 4)]))
    assert lib.hcm_op_embed_rows(_ptr(ed), _ptr(idd), y.ptr(), 7, 32, 40, 9, 5, None) == ERR_ARG          # col0 + D > ld


def test_val_subtask_follows_the_trainers_masked_fill():
    lib, _ = _lib()
    nst, rows = 3, 70                     # two workgroups
    o = torch.tensor([-1, 0, 1, 2, 3, 4, 5, 1 << 40, -(1 << 40), 3] * 7)
    want = torch.where((o >= 1) & (o <= nst), o - 1, torch.full_like(o, nst))
    valid = (o >= 0) & (o <= nst)
    assert torch.equal(want[valid], (o - 1).masked_fill(o == 0, nst)[valid])        # hierarchical_trainer.py:597-599 on the labels it can hold
    od, sub = _dev(o), Out(rows, 1, torch.int64)
    assert lib.hcm_op_val_subtask(_ptr(od), sub.ptr(), rows, nst, None) == 0
    assert torch.equal(sub.check()[:, 0], want)


@pytest.mark.parametrize("prec", PRECS)
def test_fill_cols_is_one_rounding(prec):
    lib, _ = _lib()
    B, S, Cc, ld = 2, 5, 64, 80
    tab = sc.uni(sc.gen(4), S, Cc) * 3
    y = Out(B * S, ld, sc.TDT[prec], col0=8, cols=Cc)
    td = _dev(tab)
    assert lib.hcm_op_fill_cols(_ptr(td), y.ptr(8), sc.CODE[prec], B, S, Cc, ld, None) == 0
    assert torch.equal(_bits(y.check().view(B, S, Cc)), _bits(tab.to(sc.TDT[prec])[None].expand(B, S, Cc)))


@pytest.mark.parametrize("cols", [70, 300])
@pytest.mark.parametrize("n_src", [5, 1])
def test_copy_rows_copies_or_broadcasts(n_src, cols):
    lib, _ = _lib()
    rows = 5
    src = sc.uni(sc.gen(cols), n_src, cols)
    sd = _padded(src, 3)
    dst = Out(rows, cols + 5, cols=cols)
    assert lib.hcm_op_copy_rows(_ptr(sd), cols + 3, n_src, dst.ptr(), cols + 5, rows, cols, None) == 0
    assert torch.equal(_bits(dst.check()), _bits(src.expand(rows, cols) if n_src == 1 else src))
    assert lib.hcm_op_copy_rows(_ptr(sd), cols + 3, 3, dst.ptr(), cols + 5, rows, cols, None) == ERR_ARG       # 1 < n_src < rows


@pytest.mark.parametrize("H", [96, 256])
@pytest.mark.parametrize("kind", [sc.LSTM, sc.GRU], ids=["lstm", "gru"])
def test_instr_cell_matches_the_packed_step(kind, H):
    """lengths 4 9 1 at steps 0, 3, 4, 8: an active sample steps, an inactive one keeps the bits of its state and emits exact zeros; only the
    H columns at col0 of the step's own rows are written"""
    lib, _ = _lib()
    B, L, G = 3, 9, 4 if kind == sc.LSTM else 3
    g = sc.gen(H + kind)
    pre, gh = sc.uni(g, B * L, G * H, lo=-3, hi=3), sc.uni(g, B, G * H, lo=-3, hi=3)
    h0, c0 = sc.uni(g, B, H), sc.uni(g, B, H, lo=-2, hi=2)
    lengths = torch.tensor([4, 9, 1], dtype=torch.int32)
    pd, gd, ld_ = _dev(pre), _dev(gh), _dev(lengths)
    ld_out, col0 = 2 * H + 4, H

    def launch(t, b0=0, Bn=B):
        h, c = _dev(h0[b0:b0 + Bn]), (_dev(c0[b0:b0 + Bn]) if kind == sc.LSTM else None)
        out = Out(Bn * L, ld_out, col0=col0, cols=H, rows_sel=[b * L + t for b in range(Bn)])
        assert lib.hcm_op_instr_cell(_ptr(pd, b0 * L * G * H), _ptr(gd, b0 * G * H), _ptr(h), _ptr(c), _ptr(ld_, b0), out.ptr(), t, Bn, L, H, ld_out, col0,
                                     kind, None) == 0
        return h.cpu(), (c.cpu() if c is not None else None), out.check()
    for t in (0, 3, 4, 8):
        h, c, out = launch(t)
        act = t < lengths
        rh, rc, ro = sc.instr_cell_ref(kind, pre.view(B, L, -1)[:, t], gh, h0, c0 if kind == sc.LSTM else None, act)
        name = f"{'lstm' if kind == sc.LSTM else 'gru'} H{H} t{t}"
        _f32_check("instr_cell h", name, h, rh)
        _f32_check("instr_cell out", name, out, ro)
        if kind == sc.LSTM:
            _f32_check("instr_cell c", name, c, rc)
        idle = ~act
        assert bool(idle.any()) == (t >= 1)
        assert torch.equal(_bits(h[idle]), _bits(h0[idle])) and bool((_bits(out[idle]) == 0).all())
        if kind == sc.LSTM:
            assert torch.equal(_bits(c[idle]), _bits(c0[idle]))
        assert torch.equal(_bits(out[act]), _bits(h[act]))
        h2, c2, out2 = launch(t)
        assert torch.equal(_bits(h2), _bits(h)) and torch.equal(_bits(out2), _bits(out))
        for b in range(B):
            h1, c1, o1 = launch(t, b, 1)
            assert torch.equal(_bits(h1), _bits(h[b:b + 1])) and torch.equal(_bits(o1), _bits(out[b:b + 1])), b
    z = torch.zeros(16, device="cuda")
    assert lib.hcm_op_instr_cell(_ptr(z), _ptr(z), _ptr(z), _ptr(z) if kind == sc.LSTM else None, _ptr(ld_), _ptr(z), 9, 3, 9, 4, 4, 0, kind, None) == ERR_ARG   # t = L
    assert lib.hcm_op_instr_cell(_ptr(z), _ptr(z), _ptr(z), None if kind == sc.LSTM else _ptr(z), _ptr(ld_), _ptr(z), 0, 3, 9, 4, 4, 0, kind, None) == ERR_ARG   # c and the cell type disagree
