"""Cases of the two instruction-stream kernels (csrc/features.hip: instr_feat_ingest / instr_feat_export behind hcm_op_instr_feat_*) and the
CPU side of what they must give: torch's own `.to(dtype)` on the mapped rows, zeros behind a length.

A case is (B, src_rows, L, D, lens, offset): output row r reads source row r % src_rows; `offset` shifts BOTH pointers by that many elements
(one element off 16-byte alignment: the launcher must take the scalar form)."""
import torch

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
GUARD = 64           # elements in front of and behind every output buffer that no launch may touch
FILL = 7.0           # what the guards and the output are pre-filled with

CASES = {
    "one_position": (1, 1, 1, 768, None, 0),                      # a single 768-wide position: less than one workgroup of chunks
    "chunk_ragged": (6, 2, 5, 768, [5, 1, 3, 5, 2, 4], 0),        # time-major (N = 2): row t*2 + n <- stream n; more than one workgroup per row
    "one_for_all": (6, 1, 3, 256, [3, 2, 1, 3, 1, 2], 0),         # one instruction for every row
    "scalar_width": (4, 4, 7, 100, [7, 1, 4, 6], 0),              # D no multiple of 8: the scalar form
    "scalar_misaligned": (3, 3, 12, 768, [12, 5, 1], 1),          # D fits, both pointers one element off: the scalar form through misalignment
}

# values that round differently in fp16 and bf16 (1 + 2^-9 is a tie in bf16 and exact in fp16; 1 + 2^-11 a tie in fp16), both ends of fp16's
# range, values past it (fp16: inf, bf16: finite), an fp16 subnormal, an f32 subnormal, signed zeros and infinities
SPECIALS = [1.0 + 2.0 ** -9, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -9, -(1.0 + 2.0 ** -8 + 2.0 ** -12), 65504.0, -65504.0, 65520.0, -65519.0, 70000.0,
            2.0 ** -24, -3 * 2.0 ** -24, 6.0e-8, 1.0e-40, -1.0e-40, 0.0, -0.0, float("inf"), float("-inf"), 3.3895314e38, 0.1, -1.0 / 3.0]


def source(name):
    """f32 (src_rows, L, D) of a case: random values with the specials spread over it, the same for every dtype"""
    _, src_rows, L, D, _, _ = CASES[name]
    g = torch.Generator().manual_seed(len(name) + 31 * D)
    x = (torch.randn(src_rows, L, D, generator=g) * 3).contiguous()
    flat = x.view(-1)
    stride = max(1, flat.numel() // (3 * len(SPECIALS)))
    for i in range(3 * len(SPECIALS)):
        if i * stride < flat.numel():
            flat[i * stride] = SPECIALS[i % len(SPECIALS)]
    return x


def mapped(x, B):
    """(B, L, D): output row r <- source row r % src_rows"""
    return x[torch.arange(B) % x.shape[0]]


def expected(x, B, dtype, lens):
    """what the ingest must write: torch's conversion of the mapped rows, exact +0.0 behind each length"""
    y = mapped(x, B).to(DTYPES[dtype])
    if lens is not None:
        for r, n in enumerate(lens):
            y[r, n:] = 0
    return y


def bits(t):
    """a tensor's storage as integers, so that -0.0 / +0.0 and NaN payloads compare as what they are"""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)
