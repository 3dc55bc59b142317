"""Record the bits of the instruction encoder's forward scans: tests/golden/instr_scan_parent_bits.json, which
tests/test_instr_train_gpu.py::test_forward_scans_carry_the_parent_commits_bits holds every later commit to.

Per case of tests/instr_train_cases.py PARENT_BITS_CASES: hcm_op_instr_scan_train on inputs drawn from a seeded CPU generator, then
hcm_op_instr_scan_infer on the `work` buffer that call packed -- the C ABI only.  Every output starts as NaN; the file holds the SHA-256 of the
raw bytes of out, fin, gates, c_seq and the inference out, and of every input.  Run it on the GPU with the library built from the commit whose bits
are to be kept (the fixture in the tree was recorded in front of the one-kernel scan of csrc/instr_scan.hip):

    python tools/record_instr_scan_bits.py [--out tests/golden/instr_scan_parent_bits.json]
"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import hcm_pkg; hcm_pkg.load()
from robo_vln_amd import _lib
from tests import instr_train_cases as cases

out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "tests", "golden", "instr_scan_parent_bits.json")
if not torch.cuda.is_available():
    raise SystemExit("record_instr_scan_bits.py records on the GPU; none is visible")
rec = {}
for case in cases.PARENT_BITS_CASES:
    inputs, outputs = cases.forward_scan_digests(_lib.lib(), *case)
    rec[cases.case_id(*case)] = {"inputs": inputs, "outputs": outputs}
    print(cases.case_id(*case), outputs["out"][:12])
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump({"hash": "sha256 of the raw bytes, outputs pre-filled with NaN", "torch": torch.__version__, "cases": rec}, f, indent=1)
    f.write("\n")
print(f"wrote {len(rec)} cases to {out_path}")
