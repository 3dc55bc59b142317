"""Fused bottleneck tail (3x3 conv -> 1x1 expansion + identity, one launch) vs the two stand-alone conv launches, bf16.
usage: python tools/bneck_bench.py [B H C1 stride]
       python tools/bneck_bench.py stage     the stage transition layer2 -> layer3 at the bench shape (128 images, 32 x 32, 128 mid channels): the last
                                             block + layer3's first reduction (512 -> 256) as one launch against the two launches it replaces, three
                                             repeats of the 100 warm-up + 200 timed protocol and their spread
       python tools/bneck_bench.py first     the stage transition layer1 -> layer2 (128 images, 64 x 64, stride 2): layer2 block 0 with its 256 -> 512
                                             down-sample conv folded into the expansion GEMM against the down-sample launch + the block launch"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import hcm_pkg; hcm_pkg.load()
from robo_vln_amd import _lib
lib = _lib.lib()
STAGE = len(sys.argv) >= 2 and sys.argv[1] == "stage"
FIRST = len(sys.argv) >= 2 and sys.argv[1] == "first"


def once(fn):
    for _ in range(100): assert fn() == 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 200 * 1e3


def report(tag, res):
    for name, v in res.items():
        print(f"{tag}: {name:24s} " + " ".join(f"{t:7.1f}" for t in v) + f" us  (spread {max(v) - min(v):.1f})")
    a, b = list(res.values())
    print(f"gain {min(a) - max(b):.1f} .. {max(a) - min(b):.1f} us")


if FIRST:
    # layer2 block 0 at the bench shape: 128 images, 64 x 64 block input (256 channels) and mid tensor (128), stride 2
    CODE, tdt, P = _lib.HCM_F16, torch.float16, (lambda t: t.data_ptr())
    B, H, C1, Cd, C3, CN = 128, 64, 128, 256, 512, 128
    Ho = H // 2
    r = lambda *s: torch.randn(*s, device="cuda")
    x, xd = r(B, H, H, C1).to(tdt), r(B, H, H, Cd).to(tdt)
    w2, b2 = (r(C1, 9 * C1) * 0.05).to(tdt), r(C1)
    w3, b3, wd, bd = (r(C3, C1) * 0.05).to(tdt), r(C3), (r(C3, Cd) * 0.05).to(tdt), r(C3)
    w1, b1 = (r(CN, C3) * 0.05).to(tdt), r(CN)
    w3ds, b3ds = torch.cat([w3, wd], 1).contiguous(), b3 + bd
    idt = torch.empty(B, Ho, Ho, C3, device="cuda", dtype=tdt); y = torch.empty_like(idt); o1 = torch.empty(B, Ho, Ho, CN, device="cuda", dtype=tdt)
    def separate():
        lib.hcm_op_conv2d(P(xd), P(wd), P(bd), None, P(idt), CODE, B, H, H, Cd, C3, 1, 1, 2, 0, 0, None)
        return lib.hcm_op_bottleneck_tail_next(P(x), P(w2), P(b2), P(w3), P(b3), P(idt), P(y), P(w1), P(b1), P(o1), CODE, B, H, H, C1, 2, CN, None)
    folded = lambda: lib.hcm_op_bottleneck_stage(P(x), P(w2), P(b2), P(w3ds), P(b3ds), None, P(xd), P(y), P(w1), P(b1), P(o1), CODE, B, H, H, C1, 2, CN, 4, 1, None)
    res = {"down-sample + block launch": [], "one launch": []}
    for rep in range(3):
        res["down-sample + block launch"].append(once(separate))
        res["one launch"].append(once(folded))
    report(f"B={B} {C1}ch @{H} stride 2, {Cd}-channel down-sample folded", res)
    sys.exit(0)
if STAGE:
    os.environ["BNECK_CN"] = "256"
    sys.argv = sys.argv[:1] + ["128", "32", "128", "1"]
cases = [[int(v) for v in sys.argv[1:5]]] if len(sys.argv) >= 5 else [[128, 64, 64, 1], [128, 32, 128, 1], [128, 64, 128, 2]]
CODE, tdt = (CODE, torch.bfloat16) if os.environ.get("BNECK_DT") == "bf16" else (_lib.HCM_F16, torch.float16)
P = lambda t: t.data_ptr()
for B, H, C1, stride in cases:
    C3 = 4 * C1
    Ho = (H + 2 - 3) // stride + 1
    x = torch.randn(B, H, H, C1, device="cuda").to(tdt)
    w2 = (torch.randn(C1, 3, 3, C1, device="cuda") * 0.05).to(tdt); b2 = torch.randn(C1, device="cuda")
    w3 = (torch.randn(C3, 1, 1, C1, device="cuda") * 0.05).to(tdt); b3 = torch.randn(C3, device="cuda")
    r = torch.randn(B, Ho, Ho, C3, device="cuda").to(tdt); y = torch.empty_like(r); mid = torch.empty(B, Ho, Ho, C1, device="cuda", dtype=tdt)
    fused = lambda: lib.hcm_op_bottleneck_tail(P(x), P(w2), P(b2), P(w3), P(b3), P(r), P(y), CODE, B, H, H, C1, stride, None)
    def two():
        lib.hcm_op_conv2d(P(x), P(w2), P(b2), None, P(mid), CODE, B, H, H, C1, C1, 3, 3, stride, 1, 1, None)
        return lib.hcm_op_conv2d(P(mid), P(w3), P(b3), P(r), P(y), CODE, B, Ho, Ho, C1, C3, 1, 1, 1, 0, 1, None)
    CN = int(os.environ.get('BNECK_CN', C1))
    w1 = (torch.randn(CN, 1, 1, C3, device="cuda") * 0.05).to(tdt); b1 = torch.randn(CN, device="cuda"); o1 = torch.empty(B, Ho, Ho, CN, device="cuda", dtype=tdt)
    fused3 = lambda: lib.hcm_op_bottleneck_tail_next(P(x), P(w2), P(b2), P(w3), P(b3), P(r), P(y), P(w1), P(b1), P(o1), CODE, B, H, H, C1, stride, CN, None)
    def three():
        fused()
        return lib.hcm_op_conv2d(P(y), P(w1), P(b1), None, P(o1), CODE, B, Ho, Ho, C3, CN, 1, 1, 1, 0, 1, None)
    if STAGE:
        def once(fn):
            for _ in range(100): assert fn() == 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200): fn()
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1) / 200 * 1e3
        res = {"tail + reduction launch": [], "one launch": []}
        for rep in range(3):
            res["tail + reduction launch"].append(once(three))
            res["one launch"].append(once(fused3))
        for name, v in res.items():
            print(f"B={B} {C1}ch @{H} -> {CN}: {name:24s} " + " ".join(f"{t:7.1f}" for t in v) + f" us  (spread {max(v) - min(v):.1f})")
        a, b = res["tail + reduction launch"], res["one launch"]
        print(f"gain {min(a) - max(b):.1f} .. {max(a) - min(b):.1f} us")
        continue
    for name, fn in (("two launches", two), ("fused", fused), ("fused + next c1", three), ("fused incl. c1", fused3)):
        for _ in range(100): assert fn() == 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200): fn()
        e1.record(); torch.cuda.synchronize()
        print(f"B={B} {C1}ch @{H} stride {stride}: {name:13s} {e0.elapsed_time(e1) / 200 * 1e3:7.1f} us")
