"""A few Seq2SeqNet steps (B = 64, 256 x 256, L = 80, "fp16", eager launches) for a kernel trace:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/s2s_one_step.py [GRU]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import hcm_pkg; hcm_pkg.load()
from robo_vln_amd.config import S2SConfig
from robo_vln_amd import synth
from robo_vln_amd.seq2seq import S2SEngine
B = 64
cfg = S2SConfig(instr_rnn=sys.argv[1] if len(sys.argv) > 1 else "LSTM").validate()
eng = S2SEngine(cfg, synth.make_s2s_weights(cfg, 0), max_batch=B, precision="fp16")
obs = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in synth.make_s2s_observations(cfg, B, rgb_uint8=True).items()}
h = torch.zeros(cfg.num_recurrent_layers, B, cfg.hidden, device="cuda"); m = torch.ones(B, device="cuda")
for _ in range(3):
    h = eng.forward(obs, h, m)[3]
torch.cuda.synchronize()
print("done")
