"""Shared cases of the differentiable instruction encoder (robo_vln_amd.train.instr_scan): inputs from a seeded generator and the float64
CPU-autograd reference through train.instr_encoder_ref, computed once per case and never modified.

Inputs: weights and biases uniform in +-0.1, embedded rows and the cotangent uniform in +-1.  A case is (rnn, dirs, final, B, L): the lengths
come from LENGTHS, the cotangent has the shape of the result -- (B, L, dirs*H), or (B, H) for the final state.  EDGE_CASES hold lengths of 0,
below 0 and past L (instr_encoder_ref's activity test is t < lengths, so they need no other reference), the 200-token horizon and eight samples
per workgroup in one direction; SATURATED_CASES are built with weight_ih times SATURATED_IH_SCALE.

scan_inputs / forward_scan_digests: the forward scans alone on inputs drawn without a GEMM, as SHA-256 digests, for the bits recorded in
tests/golden/instr_scan_parent_bits.json (PARENT_BITS_CASES)."""
import ctypes
import functools
import hashlib

import torch

from robo_vln_amd import train
from tests.vla_train_cases import rel  # noqa: F401  (the project's bound rule, shared)

BOUND = 1e-5
# (rnn_type, directions, final_state_only)
SETTINGS = [("LSTM", 2, False), ("LSTM", 1, False), ("LSTM", 1, True), ("GRU", 2, False), ("GRU", 1, False), ("GRU", 1, True)]
# lengths per (B, L): one row of one token; a length-1 row beside a full one (one workgroup, partly filled); a row of full length, a row of
# length 1 and lengths either side of 32; nine rows (an odd count: the last workgroup holds one sample); and the two shapes at which two
# directions pass 128 workgroups at two and at four samples per workgroup
LENGTHS = {
    (1, 1): (1,),
    (3, 7): (7, 1, 4),
    (5, 33): (33, 17, 1, 20, 32),
    (9, 12): (12, 3, 7, 1, 9, 12, 5, 10, 2),
    (130, 3): tuple(1 + (3 * b + b // 7) % 3 for b in range(130)),
    (260, 2): tuple(1 + (b + b // 5) % 2 for b in range(260)),
    # the edges of include/hcm.h's packed-sequence promise (EDGE_CASES below).  Rows of length 0, at two samples per workgroup a workgroup that owns
    # only such rows (rows 2 and 3: it walks no step and reads nothing), and a negative length, which counts as 0
    (6, 9): (9, 0, 0, 0, 4, -3),
    # a length past L, which counts as L
    (4, 5): (5, 9, 0, 1),
    # the documented horizon of 200 tokens, beside an empty row
    (3, 200): (200, 0, 137),
    # eight samples per workgroup with ONE direction (ceil(513 / 4) = 129 workgroups are one too many): rows 8..15 empty, so the second workgroup is
    # idle, and the last workgroup holds one sample
    (513, 2): tuple(0 if 8 <= b < 16 else 1 + (b + b // 5) % 2 for b in range(513)),
    # the saturated regime (SATURATED_CASES below): long enough for a saturated state to be carried, with an empty row and a row of one token
    (4, 40): (40, 0, 23, 1),
}
# the settings each edge shape runs with: all six where the scan is short, four at the horizon, the one-direction three at 513 rows
EDGE_SETTINGS = {
    (6, 9): SETTINGS,
    (4, 5): SETTINGS,
    (3, 200): [("LSTM", 2, False), ("GRU", 1, True), ("GRU", 2, False), ("LSTM", 1, True)],
    (513, 2): [("LSTM", 1, True), ("GRU", 1, True), ("LSTM", 1, False)],
    # four samples per workgroup with ONE direction (257 .. 512 rows), which the two-direction cases of this shape do not reach
    (260, 2): [("LSTM", 1, True), ("GRU", 1, False)],
}
# the cases of tests/test_instr_train_gpu.py in front of the edges: every setting at the four small shapes, two directions at the two large ones
GPU_SHAPES = [(1, 1), (3, 7), (5, 33), (9, 12)]
GPU_CASES = [(*s, B, L) for s in SETTINGS for B, L in GPU_SHAPES] + [(rnn, 2, False, B, L) for rnn in ("LSTM", "GRU") for B, L in ((130, 3), (260, 2))]
EDGE_CASES = [(*s, B, L) for (B, L), settings in EDGE_SETTINGS.items() for s in settings]
# weight_ih times 20, uniform in +-2: about a fifth of the input-side pre-activations pass +-6, where g (1 - g) and 1 - n^2 round towards zero
SATURATED_IH_SCALE = 20.0
SATURATED_CASES = [("LSTM", 2, False, 4, 40), ("GRU", 2, False, 4, 40)]
PARAM_NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
# the training forward against the engines' one-launch scans, bit for bit (the inference hook serves the final-state scan of either cell and the
# per-token scan of the LSTM)
INFER_EDGES = [s + shape for shape in ((6, 9), (3, 200), (513, 2)) for s in EDGE_SETTINGS[shape] if s[2] or s[0] == "LSTM"]
INFER_CASES = [("LSTM", 1, True, 5, 33), ("GRU", 1, True, 5, 33), ("LSTM", 1, True, 9, 12), ("GRU", 1, True, 9, 12), ("LSTM", 2, False, 5, 33),
               ("LSTM", 1, False, 9, 12), ("LSTM", 2, False, 130, 3), ("LSTM", 2, False, 260, 2)] + INFER_EDGES
# the forward scans against the bits recorded at the commit in front of the one-kernel scan (tests/golden/instr_scan_parent_bits.json, written by
# tools/record_instr_scan_bits.py): INFER_CASES and two per-token GRU cases, which only the training forward runs.  Two, four and eight samples
# per workgroup, both cells, one and two directions, partial and empty workgroups, lengths below 0 and past L.
PARENT_BITS_CASES = INFER_CASES + [("GRU", 2, False, 5, 33), ("GRU", 2, False, 260, 2)]


def grad_names(dirs):
    return ["d_emb"] + [f"d_{n}{sfx}" for sfx in ("", "_reverse")[:dirs] for n in PARAM_NAMES]


def make_inputs(rnn, dirs, final, B, L, H, E, seed, ih_scale=1.0):
    """(embedded (B, L, E), params per direction, cotangent), float32 on the CPU; ih_scale multiplies every weight_ih behind the draws, so that
    every other tensor of a seed is the same with and without it"""
    g = torch.Generator().manual_seed(seed)

    def u(*shape, scale=1.0):
        return (torch.rand(*shape, generator=g) * 2 - 1) * scale

    G = 4 if rnn == "LSTM" else 3
    params = [(u(G * H, E, scale=0.1), u(G * H, H, scale=0.1), u(G * H, scale=0.1), u(G * H, scale=0.1)) for _ in range(dirs)]
    emb = u(B, L, E)
    cot = u(B, H) if final else u(B, L, dirs * H)
    if ih_scale != 1.0:
        params = [(w_ih * ih_scale, w_hh, b_ih, b_hh) for w_ih, w_hh, b_ih, b_hh in params]
    return emb, params, cot


def clamped(lengths, L):
    """the lengths as the kernels read them: below 0 counts as 0, past L as L"""
    return lengths.clamp(0, L)


def reference(emb, lengths, params, final, cot):
    """float64 CPU autograd through instr_encoder_ref: (result, gradients in grad_names order)"""
    e64 = emb.double().requires_grad_()
    p64 = [tuple(t.double().requires_grad_() for t in p) for p in params]
    y = train.instr_encoder_ref(e64, lengths, p64, final)
    leaves = [e64] + [t for p in p64 for t in p]
    return y.detach(), torch.autograd.grad(y, leaves, cot.double())


@functools.lru_cache(maxsize=None)
def case(rnn, dirs, final, B, L, H=256, E=50, ih_scale=1.0):
    lengths = torch.tensor(LENGTHS[(B, L)])
    emb, params, cot = make_inputs(rnn, dirs, final, B, L, H, E, 10000 * B + 100 * L + 10 * dirs + 2 * final + (rnn == "GRU"), ih_scale)
    y64, g64 = reference(emb, lengths, params, final, cot)
    return dict(emb=emb, params=params, cot=cot, lengths=lengths, y64=y64, ref=dict(zip(grad_names(dirs), g64)))


def saved64(emb, lengths, params):
    """What the training forward saves, from a float64 cell loop: gates (dirs, B, L, 4H) -- LSTM i,f,g,o; GRU r,z,n and hn = W_hn h + b_hn -- and
    c (dirs, B, L, H) (LSTM; None for GRU), NaN at inactive tokens; and the boolean activity mask (B, L)."""
    B, L = emb.shape[0], emb.shape[1]
    H = params[0][1].shape[1]
    lstm = params[0][1].shape[0] == 4 * H
    x = emb.double()
    gates = torch.full((len(params), B, L, 4 * H), float("nan"), dtype=torch.float64)
    cs = torch.full((len(params), B, L, H), float("nan"), dtype=torch.float64) if lstm else None
    for d, p in enumerate(params):
        w_ih, w_hh, b_ih, b_hh = (t.double() for t in p)
        for b in range(B):
            h, c = torch.zeros(H, dtype=torch.float64), torch.zeros(H, dtype=torch.float64)
            n = min(max(int(lengths[b]), 0), L)
            for t in (range(n - 1, -1, -1) if d else range(n)):
                gi, gh = w_ih @ x[b, t] + b_ih, w_hh @ h + b_hh
                if lstm:
                    i, f, g, o = (gi + gh).chunk(4)
                    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
                    c = f * c + i * g
                    h = o * torch.tanh(c)
                    gates[d, b, t] = torch.cat([i, f, g, o])
                    cs[d, b, t] = c
                else:
                    (i_r, i_z, i_n), (h_r, h_z, h_n) = gi.chunk(3), gh.chunk(3)
                    r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
                    nn_ = torch.tanh(i_n + r * h_n)
                    h = (1 - z) * nn_ + z * h
                    gates[d, b, t] = torch.cat([r, z, nn_, h_n])
    active = torch.arange(L)[None, :] < lengths[:, None]
    return gates, cs, active


def scan_inputs(rnn, dirs, B, L, H=256):
    """The scan's own inputs, drawn directly (no GEMM, so no BLAS library has a say in their bits), float32 on the CPU: pre (dirs, B*L, G*H)
    uniform in +-1, w_hh (dirs, G*H, H) and b_hn (dirs, H; None for LSTM) uniform in +-0.1, and LENGTHS[(B, L)] as int32."""
    g = torch.Generator().manual_seed(77000000 + 10000 * B + 100 * L + 10 * dirs + (rnn == "GRU"))
    G = 4 if rnn == "LSTM" else 3
    pre = torch.rand(dirs, B * L, G * H, generator=g) * 2 - 1
    w_hh = (torch.rand(dirs, G * H, H, generator=g) * 2 - 1) * 0.1
    b_hn = None if rnn == "LSTM" else (torch.rand(dirs, H, generator=g) * 2 - 1) * 0.1
    return dict(pre=pre, w_hh=w_hh, b_hn=b_hn, lengths=torch.tensor(LENGTHS[(B, L)], dtype=torch.int32))


def digest(t):
    """SHA-256 of a tensor's raw bytes (None for no tensor)"""
    return None if t is None else hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def forward_scan_digests(lib, rnn, dirs, final, B, L, H=256):
    """One case of PARENT_BITS_CASES on the GPU through the C ABI alone: hcm_op_instr_scan_train on scan_inputs, then hcm_op_instr_scan_infer (where
    it serves the case) on the `work` buffer the training call packed.  Every output starts as NaN, so an element left unwritten counts.
    Returns (input digests, output digests)."""
    from robo_vln_amd import _lib
    lstm = rnn == "LSTM"
    kind = _lib.HCM_LSTM if lstm else _lib.HCM_GRU
    inp = scan_inputs(rnn, dirs, B, L, H)
    dev = {k: None if v is None else v.cuda() for k, v in inp.items()}
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pt = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    nan = float("nan")
    o = dict(out=torch.full((B, L, dirs * H), nan, device="cuda"), fin=torch.full((B, H), nan, device="cuda"),
             gates=torch.full((dirs, B, L, 4 * H), nan, device="cuda"), c_seq=torch.full((dirs, B, L, H), nan, device="cuda") if lstm else None,
             infer_out=None)
    work = torch.empty(lib.hcm_op_instr_scan_work_floats(B, L, dirs, kind), device="cuda")
    assert lib.hcm_op_instr_scan_train(pt(dev["pre"]), pt(dev["w_hh"]), pt(dev["b_hn"]), pt(dev["lengths"]), pt(o["out"]), pt(o["fin"]), pt(o["gates"]),
                                       pt(o["c_seq"]), pt(work), B, L, H, dirs, kind, st) == 0, _lib.last_error()
    if final or lstm:
        o["infer_out"] = torch.full((B, H) if final else (B, L, dirs * H), nan, device="cuda")
        assert lib.hcm_op_instr_scan_infer(pt(dev["pre"]), pt(work), pt(dev["b_hn"]), pt(dev["lengths"]), pt(o["infer_out"]), B, L, H, dirs, kind,
                                           int(final), st) == 0, _lib.last_error()
    torch.cuda.synchronize()
    return {k: digest(v) for k, v in inp.items()}, {k: digest(v) for k, v in o.items()}


def case_id(rnn, dirs, final, B, L):
    return f"{rnn}-{dirs}-{final}-{B}-{L}"
