"""Case lists and plain float64 references for the step's small kernels (csrc/elementwise.hip through the hcm_op_* entries of include/hcm.h):
the recurrent cells with their fused heads, argmax and sub-task embedding, CMANet's one-query attention, the token pools, the two embedding
front ends, the f32-stream LayerNorm, the depth average pool and the calibration range check.  CPU only; everything is rebuilt from a seed.

The references restate the REFERENCE PROJECT's statements in float64 -- RNNStateEncoder.single_forward (state_encoder.py:72-81), CMANet._attn
(cma.py:201-209), F.adaptive_avg_pool2d, BertEmbeddings, InstructionEncoder's length rule and packed step (instruction_encoder.py:70-92),
torch.argmax -- never the kernels; tests/test_step_ops_cpu.py ties them to oracle/hcm_oracle.py to 1e-12.  For 16-bit storage a reference runs
on the stored (rounded) inputs."""
import math

import torch
import torch.nn.functional as F

TDT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
CODE = {"fp32": 0, "bf16": 1, "fp16": 5}                  # HCM_F32 / HCM_BF16 / HCM_F16
IDS = {"i64": (3, torch.int64), "i32": (2, torch.int32), "f32": (0, torch.float32)}
MANT = {"fp16": 10, "bf16": 7}                             # stored mantissa bits
TINY = {"fp16": 2.0 ** -24, "bf16": 2.0 ** -133}           # subnormal spacing: the absolute floor of the one-ulp bound
F32_REL = 1e-5                                             # f32 outputs: of the tensor's largest element (README: "bound 1e-5")
LSTM, GRU = 0, 1


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def uni(g, *shape, lo=-1.0, hi=1.0):
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def stored(t, prec):
    """t rounded to the storage type: (what the device holds, the same values in float64)"""
    s = t.to(TDT[prec])
    return s, s.double()


def ulp(ref, prec):
    """spacing of the storage type at each float64 value of ref, not below its subnormal spacing"""
    a = ref.abs().clamp_min(TINY[prec])
    return torch.maximum(torch.exp2(torch.floor(torch.log2(a)) - MANT[prec]), torch.full_like(a, TINY[prec]))


def f32_bound(ref):
    return F32_REL * ref.abs().max().item()


# ------------------------------------------------------------------------------------------------ recurrent cell + heads
# (r0, r1, r2), fused pred; emb_rows = 5 with pred: r0 = 64 puts most winners at or above the table, which must read the clamped row 4
HEADSETS = {"r4_pred": ((4, 0, 0), True), "r2_1": ((2, 1, 0), False), "r2_1_tanh": ((2, 1, 1), False), "r64_pred": ((64, 0, 0), True),
            "none": ((0, 0, 0), False)}
EMB_ROWS, EMB_DIM, EMB_LD = 5, 32, 40
CELL_B, CELL_H = 5, (512, 96)        # 96: no multiple of the 256-thread stride, and lanes 32..63 idle in the heads' second wave pass
CELL_MASK = (1.0, 0.0, 1.0, 1.0, 0.0)
STALE = 1.0e30                       # what a masked sample's h / c hold: finite, so that the reference's product with mask 0 is an exact 0


def head_ld(r):
    return 7 if 0 < r <= 7 else r + 3      # ld0 = 7 > r0 is the act() record's stride


class Cell:
    """one recurrent step: gate pre-activations, previous state, masks, head weights -- float32, as the device holds them"""

    def __init__(self, kind, H, headset, B=CELL_B, seed=0):
        g = gen(1000 * seed + 10 * H + kind)
        self.kind, self.H, self.B, self.headset = kind, H, B, headset
        self.R = 2 if kind == LSTM else 1
        G = 4 if kind == LSTM else 3
        self.gates = uni(g, B, G * H, lo=-3.0, hi=3.0)
        self.gh = uni(g, B, G * H, lo=-3.0, hi=3.0) if kind == GRU else None
        self.h_in = uni(g, self.R, B, H, lo=-2.0, hi=2.0)
        self.mask = torch.tensor([CELL_MASK[b % len(CELL_MASK)] for b in range(B)])
        for b in range(B):
            if self.mask[b] == 0:
                self.h_in[:, b] = STALE * torch.sign(self.h_in[:, b])
        (self.r, self.pred) = HEADSETS[headset]
        self.w = [uni(g, r, H) / math.sqrt(H) * 3 for r in self.r]
        self.b = [uni(g, r) for r in self.r]
        self.emb = uni(g, EMB_ROWS, EMB_DIM)

    def row(self, b):
        """sample b alone, as a batch of one"""
        c = Cell.__new__(Cell)
        c.__dict__.update(self.__dict__)
        c.B = 1
        c.gates, c.h_in, c.mask = self.gates[b:b + 1].clone(), self.h_in[:, b:b + 1].clone(), self.mask[b:b + 1].clone()
        c.gh = self.gh[b:b + 1].clone() if self.gh is not None else None
        return c


def cell_ref(kind, gates, gh, h_in, mask):
    """RNNStateEncoder.single_forward behind the gate products, float64: hidden * mask, one nn.LSTM / nn.GRU step, repack.  gates (LSTM) is
    x W_ih^T + b_ih + (h*mask) W_hh^T + b_hh; gates, gh (GRU) the two products with their biases.  Returns the new hidden (R, B, H)."""
    m = mask.double().view(-1, 1)
    if kind == LSTM:
        c = h_in[1].double() * m
        i, f, gg, o = gates.double().chunk(4, dim=1)
        c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        return torch.stack([torch.sigmoid(o) * torch.tanh(c2), c2], 0)
    h = h_in[0].double() * m
    ir, iz, inn = gates.double().chunk(3, dim=1)
    hr, hz, hn = gh.double().chunk(3, dim=1)
    r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
    return ((1 - z) * torch.tanh(inn + r * hn) + z * h)[None]


def heads_ref(h, w, b):
    """nn.Linear on the new hidden state per head, the third behind a tanh (Seq2SeqNet's progress monitor, seq2seq.py:177); float64"""
    out = [F.linear(h.double(), w[i].double(), b[i].double()) for i in range(3)]
    out[2] = torch.tanh(out[2])
    return out


def rnn_prep_ref(h_in, mask):
    """hidden[0] * mask in float32: ONE product, so the device must match it to the bit"""
    return h_in[0] * mask.view(-1, 1)


# ------------------------------------------------------------------------------------------------ packed instruction step
def instr_cell_ref(kind, pre_t, gh, h, c, active):
    """one step of nn.LSTM / nn.GRU over pack_padded_sequence, float64: an active sample steps, an inactive one keeps its state and emits 0.
    pre_t, gh (B, G*H) as include/hcm.h gives them; returns (h', c' or None, out)."""
    a = active.view(-1, 1)
    pre_t, gh, h = pre_t.double(), gh.double(), h.double()
    if kind == GRU:
        ir, iz, inn = pre_t.chunk(3, dim=1)
        hr, hz, hn = gh.chunk(3, dim=1)
        r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
        h2 = (1 - z) * torch.tanh(inn + r * hn) + z * h
        return torch.where(a, h2, h), None, torch.where(a, h2, torch.zeros_like(h2))
    i, f, gg, o = (pre_t + gh).chunk(4, dim=1)
    c2 = torch.sigmoid(f) * c.double() + torch.sigmoid(i) * torch.tanh(gg)
    h2 = torch.sigmoid(o) * torch.tanh(c2)
    return torch.where(a, h2, h), torch.where(a, c2, c.double()), torch.where(a, h2, torch.zeros_like(h2))


# ------------------------------------------------------------------------------------------------ one-query attention
# (B, S, D, Dv, interleaved k | v, lengths or None)
ATTN_CASES = [(3, 1, 64, 32, False, None), (4, 80, 256, 512, False, None), (4, 80, 256, 512, False, (1, 80, 37, 64)),
              (2, 200, 100, 36, False, None), (2, 200, 100, 36, False, (200, 3)), (2, 16, 256, 2112, True, None)]


def attn_id(c):
    return f"B{c[0]}_S{c[1]}_D{c[2]}_Dv{c[3]}" + ("_kv" if c[4] else "") + ("_lens" if c[5] else "")


def make_attn(case, seed=0):
    B, S, D, Dv, inter, lens = case
    g = gen(seed + S + D)
    q, k, v = uni(g, B, D), uni(g, B, S, D), uni(g, B, S, Dv)
    return q, k, v, (torch.tensor(lens, dtype=torch.int32) if lens else None), D ** -0.5


def attn_ref(q, k, v, lengths, scale, probs=False):
    """CMANet._attn: logits = q . k_s, minus 1e8 at the masked positions (s >= length), THEN times scale, softmax, weighted sum of v; float64"""
    logits = torch.einsum("nc,nsc->ns", q.double(), k.double())
    if lengths is not None:
        masked = torch.arange(k.shape[1])[None] >= lengths.long()[:, None]
        logits = logits - masked.double() * 1e8
    p = F.softmax(logits * scale, dim=1)
    return p if probs else torch.einsum("ns,nsc->nc", p, v.double())


# ------------------------------------------------------------------------------------------------ pools
POOL_CASES = [(8, 8, 4, 4), (5, 7, 4, 4), (2, 2, 4, 4), (4, 6, 1, 1), (4, 4, 4, 4)]       # H, W, OH, OW
POOL_B, POOL_C = 3, 64               # 3 * 16 * 64 / 8 = 384 chunks: two workgroups even at 16-bit


def pool_windows(n, o):
    """adaptive_avg_pool's windows along one axis: [floor(i n / o), ceil((i + 1) n / o))"""
    return [((i * n) // o, -((-(i + 1) * n) // o)) for i in range(o)]


def make_pool_input(B, H, W, C, prec, seed=0):
    """a ReLU output, as every pooled map of the trunks is: non-negative, a third of it exact zeros.  (B, H, W, C) NHWC"""
    g = gen(seed + 31 * H + W)
    x = uni(g, B, H, W, C, lo=-0.5, hi=1.0).clamp_min(0.0)
    return stored(x, prec)


def adaptive_pool_ref(x64, OH, OW):
    """F.adaptive_avg_pool2d on the NHWC float64 map"""
    return F.adaptive_avg_pool2d(x64.permute(0, 3, 1, 2), (OH, OW)).permute(0, 2, 3, 1).contiguous()


MEAN_CASES = [(3, 16, 64, None), (2, 80, 256, (80, 1)), (4, 37, 256, (37, 5, 0, 100))]     # B, S, C, lens


def mean_rows_ref(x64, lens):
    """AdaptiveAvgPool1d(1) over the first clamp(len, 1, S) tokens of each sample (include/hcm.h states the clamp); x64 (B, S, C)"""
    B, S, _ = x64.shape
    n = [S] * B if lens is None else [min(max(int(l), 1), S) for l in lens]
    return torch.stack([x64[b, :n[b]].mean(0) for b in range(B)])


AVGPOOL2_CASES = [(2, 8, 12), (1, 64, 64)]


def avgpool2_ref(x):
    return F.avg_pool2d(x.double()[:, None], 2)[:, 0]


# ------------------------------------------------------------------------------------------------ embedding front ends
BERT_VOCAB, BERT_MAXPOS = 50, 16
BERT_IDS = {7: [[0, 49, -3, 55, 5, 17, 30], [1, 2, 3, 48, 49, 0, 7]], 1: [[49], [-3]]}      # 0, vocab - 1, -3, vocab + 5: the clamp


def make_bert_tables(D, seed=0):
    g = gen(seed + D)
    return dict(word=uni(g, BERT_VOCAB, D), pos=uni(g, BERT_MAXPOS, D), type0=uni(g, D), gamma=uni(g, D, lo=0.8, hi=1.2), beta=uni(g, D, lo=-0.2, hi=0.2))


def bert_embed_ref(ids, t, eps=1e-12):
    """BertEmbeddings.forward, float64: word[id] + position[l] + token_type[0] -> LayerNorm.  ids clamped to [0, vocab - 1] first"""
    ids = ids.long().clamp(0, t["word"].shape[0] - 1)
    L, D = ids.shape[1], t["word"].shape[1]
    x = t["word"].double()[ids] + t["pos"].double()[:L][None] + t["type0"].double()[None, None]
    return F.layer_norm(x, (D,), t["gamma"].double(), t["beta"].double(), eps)


INSTR_VOCAB, INSTR_E, INSTR_LDX = 50, 50, 64
INSTR_IDS = {9: [[3, 7, 0, 9, 11, 0, 0, 0, 0], [49, 48, 47, 46, 45, 44, 43, 42, 41], [5, 0, 0, 0, 0, 0, 0, 0, 0]], 1: [[4], [0], [49]]}


def instr_lengths_ref(ids):
    """InstructionEncoder.forward: lengths = (instruction != 0.0).long().sum(dim=1) -- a zero id in the middle is simply not counted"""
    return (ids != 0).long().sum(dim=1)


def instr_embed_ref(ids, table, ldx):
    x = torch.zeros(ids.shape[0], ids.shape[1], ldx)
    x[:, :, :table.shape[1]] = table[ids.long().clamp(0, table.shape[0] - 1)]
    return x


# ------------------------------------------------------------------------------------------------ LayerNorm of the f32 stream
LN_ROWS, LN_D = (1, 7, 17), (256, 512, 768)


def make_ln(rows, D, offset=0.0, seed=0):
    g = gen(seed + 7 * rows + D)
    x = torch.randn(rows, D, generator=g) + offset
    return x, uni(g, D, lo=0.8, hi=1.2), uni(g, D, lo=-0.2, hi=0.2)


def layernorm_ref(x, gamma, beta, eps=1e-12):
    """(y, mean, rstd) in float64 of the float32 rows"""
    x = x.double()
    mean = x.mean(1)
    rstd = 1.0 / torch.sqrt(x.var(1, unbiased=False) + eps)
    return F.layer_norm(x, (x.shape[1],), gamma.double(), beta.double(), eps), mean, rstd


# ------------------------------------------------------------------------------------------------ range check
ABSMAX_CASES = [(3, 100, 128), (1, 1, 1)]
FMAX = {"fp32": torch.finfo(torch.float32).max, "fp16": 65504.0, "bf16": torch.finfo(torch.bfloat16).max}


def make_absmax(rows, cols, ld, prec, poison, seed=0):
    """[rows][ld] with NaN in the pad columns (never read); poison: NaN, +inf, -inf and the largest finite value among the logical ones"""
    g = gen(seed + cols)
    x = torch.full((rows, ld), float("nan"))
    x[:, :cols] = uni(g, rows, cols, lo=-4.0, hi=4.0)
    if poison and cols >= 8:
        x[0, 3], x[1, 99], x[2, 0], x[2, 50], x[1, 7] = float("nan"), float("inf"), float("-inf"), float("nan"), -FMAX[prec]
    return x.to(TDT[prec])


def absmax_ref(x, cols):
    """(the largest finite |x| as a float32, the count of non-finite elements) over the logical columns"""
    v = x[:, :cols].float()
    fin = torch.isfinite(v)
    return (v[fin].abs().max().item() if bool(fin.any()) else 0.0), int((~fin).sum().item())


# ------------------------------------------------------------------------------------------------ argmax
ARGMAX_B, ARGMAX_LD, ARGMAX_N = 70, 7, (1, 4, 7)


def argmax_rows(n, B=ARGMAX_B):
    """B rows of n logits (values are small multiples of 1/4: exact in every format): exact ties at every pair of positions, all-equal,
    -inf entries, +inf, a NaN at index 0, a NaN above index 0, two NaNs, NaN beside +inf; the rest random with repeats"""
    inf, nan = float("inf"), float("nan")
    rows = [[1.0] * n, [-inf] * n, [0.0] * n]
    for i in range(n):
        for j in range(i + 1, n):
            r = [float(k % 3) * 0.25 for k in range(n)]
            r[i] = r[j] = 2.0                                  # the maximum twice: the first one wins
            rows.append(r)
    for i in range(n):
        base = [0.5 * ((k * 5) % 4) for k in range(n)]
        for special in (inf, nan, -inf):
            r = list(base)
            r[i] = special
            rows.append(r)
    if n >= 3:
        rows += [[0.0, nan, 1.0] + [nan] * (n - 3), [inf, 0.0, nan] + [inf] * (n - 3), [-inf] * (n - 1) + [-1.0], [inf] * (n - 1) + [nan],
                 [-inf, nan] + [inf] * (n - 2)]
    g = gen(n)
    while len(rows) < B:
        rows.append((torch.randint(0, 4, (n,), generator=g).float() * 0.25).tolist())
    return torch.tensor(rows[:B])
