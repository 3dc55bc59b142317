"""The update steps against the reference's own autograd: the case table shared by tools/gen_update_golden.py (which runs the imported reference
models in float64 and writes tests/golden/update_*.npz) and the tests, the seeded inputs every side rebuilds, the train modules run on them,
and the fixture's encoding of a tensor -- a strided subsample, max|t| and sum|t|, and four seeded +-1 projections.  Test infrastructure only."""
import contextlib
import functools
import math
import os
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cases, hcm_oracle
from robo_vln_amd import synth, train
from robo_vln_amd.config import HCMConfig
from tests import cma_seq_cases, val_ref
from tests import flat_val_ref as fv

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PROJECTIONS = 4
STEPS = 2
ADAM = dict(lr=1e-3, eps=1e-3)       # tests/test_hier_update_gpu.py: with the default eps a parameter whose gradient is round-off takes a full step
_HIER = dict(val_ref._S, rnn_type="GRU")

# name -> (kind, config, T, N, trajectory).  GRU state encoders: the reference's in-tree seq_forward raises for LSTM (oracle/cases.py:96-100).
# Frames, instructions, masks, labels and the initial state are those of the validation cases with the same T and N; so are the weights, except
# where SEEDS names another seed.
UPDATE_CASES = {
    "update_hier_T4_N2_gru": ("hier", lambda: val_ref.case("val_T4_N2_gru")[0], 4, 2, True),
    "update_hier_ablate_depth_T2_N2": ("hier", lambda: HCMConfig(**_HIER, ablate_depth=True).validate(), 2, 2, False),
    "update_cma_T4_N2": ("cma", lambda: fv.case("flatval_cma_T4_N2")[1], 4, 2, True),
    "update_cma_ablate_instr_T2_N2": ("cma", lambda: cma_seq_cases.seq_case("cma_seq_ablate_instr_T2_N2")[0], 2, 2, False),
    "update_s2s_T4_N2_gru": ("s2s", lambda: fv.case("flatval_s2s_T4_N2_gru")[1], 4, 2, False),
    "update_s2s_pm_T3_N2_gru": ("s2s", lambda: fv.case("flatval_s2s_pm_T3_N2_gru")[1], 3, 2, True),
}
# Two conditions on the draw, in the manner of tests/vla_train_cases.py and tests/subtask_ce_cases.py -- conditions on the inputs, not
# tolerances: no tensor is left out of a comparison.  Each case takes the first weight seed from cases.SEED that meets both (first_seed).
#   kink   A pre-activation within rounding of zero switches a ReLU unit on in one precision and off in another, after which that unit's rows
#          differ by a gradient, not by rounding (seed 0 of the pair: 1e-4 of a weight's largest element after two steps).  KINK_RATIO: in every
#          ReLU call of the single step and of the trajectory, the smallest non-zero |pre-activation| in float64 is at least the LARGEST
#          deviation of any of that call's float32 pre-activations from float64 (kink_margin).  A call has 1e3 .. 1.6e5 pre-activations, so its
#          largest deviation is about 4.5 standard deviations of its rounding error: a ratio of 1 already means that another machine's
#          rounding, of the same size, needs a 4.5-sigma deviation at that one element to reach the kink.
#   adam   Adam with lr / eps = 1 hands every parameter its gradient's rounding error at full size and the next step's forward sees it: float32
#          and float64 runs of the same module drift apart by about a factor of three per step (the pair on its whole chunk: 6e-7, 3e-6, 1e-5 of
#          a tensor's largest element after one, two, three steps, over twenty seeds).  So the trajectory has two steps -- the fewest after
#          which a step has seen an update -- the pair's runs on the first two steps of its chunk (TRAJECTORY_T: 3e-6 over the seeds that pass
#          the kink condition, where the whole chunk gave 4.7e-6 at best), and SEED_BOUND: the train modules' own float32 CPU run stays within
#          the half bound that tests/test_reference_grads_cpu.py asserts of their float64 run in every tensor, the single step and the
#          trajectory (conditioning).
KINK_RATIO = 1.0
SEED_BOUND = 5e-6
SEEDS = {"update_hier_T4_N2_gru": 5}          # every other case: cases.SEED, 0
# the steps of the chunk a trajectory runs on: the pair's takes the first two of its four -- half the ReLU pre-activations and half the
# recurrence for the drift to pass through; the single step keeps the whole chunk with its padded row and its reset
TRAJECTORY_T = {"update_hier_T4_N2_gru": 2}
TRAJECTORY = tuple(n for n, c in UPDATE_CASES.items() if c[4])
# the models of a case, in the order the trainer steps them, and what each keeps frozen
MODELS = {"hier": ("hi", "lo"), "cma": ("net",), "s2s": ("net",)}
FROZEN = {"hi": train.HCM_HIGH_FROZEN_PREFIXES, "lo": train.HCM_LOW_FROZEN_PREFIXES, "net": train.CMA_TRUNK_PREFIXES}
# how many loss terms a step has: [high-level CE, action, stop] or [action, stop, aux]
TERMS = 3


def case(name):
    kind, cfg, T, N, trajectory = UPDATE_CASES[name]
    return kind, cfg(), T, N, trajectory


# ---------------------------------------------------------------- NaN-proof figures
def worse(*values):
    """the largest of the values, NaN if any is NaN (Python's max drops a NaN that is not its first argument); 0.0 of none"""
    values = list(values)
    return float(np.max(values)) if values else 0.0


def over(worst, bound):
    """the entries of compare's dict that are not within the bound -- a NaN is not: `assert not over(worst, BOUND)`"""
    return {k: v for k, v in worst.items() if not v <= bound}


# ---------------------------------------------------------------- the fixture's encoding of a tensor
def stride_of(n, sub):
    return 1 if n <= sub else -(-n // sub)


def subsample(a, sub):
    """the whole flattened tensor up to `sub` elements, otherwise `sub` values (at most) at a fixed stride"""
    a = np.asarray(a, np.float64).reshape(-1)
    return a[::stride_of(a.size, sub)].copy()


def signs(key, n):
    """(PROJECTIONS, n) of +-1, drawn from the key's CRC-32: a test redraws what the recipe drew"""
    return np.random.RandomState(zlib.crc32(key.encode())).randint(0, 2, size=(PROJECTIONS, n)).astype(np.float64) * 2 - 1


def encode(key, a, sub):
    """(values, [max|a|, sum|a|, elements], projections) of one tensor, float64"""
    a = np.asarray(a, np.float64).reshape(-1)
    return subsample(a, sub), np.array([np.abs(a).max(), np.abs(a).sum(), a.size], np.float64), signs(key, a.size) @ a


def errors(key, got, values, stat, proj, sub, scale=None):
    """One tensor against its encoding, every figure as a multiple of the scale (the reference tensor's largest element unless given):
    (subsample, max|t|, sum|t| / n, projections / sqrt(n)).  The signs of a projection are independent of the errors, so a projection's error
    grows as sqrt(n) whatever the errors share; |sum|a| - sum|b|| <= sum|a - b| <= n max|a - b| is all that holds for the sum of magnitudes,
    whose errors share the upstream factors' rounding and add up.  A stored tensor of exact zeros is met exactly or not at all."""
    got = np.asarray(got, np.float64).reshape(-1)
    n = int(stat[2])
    assert got.size == n, (key, got.size, n)
    sub = subsample(got, sub)
    assert sub.shape == values.shape, (key, sub.shape, values.shape)
    scale = float(stat[0]) if scale is None else scale
    raw = (np.abs(sub - values).max(), abs(np.abs(got).max() - stat[0]), abs(np.abs(got).sum() - stat[1]) / n,
           np.abs(signs(key, n) @ got - proj).max() / math.sqrt(n))
    if scale == 0:
        return tuple(0.0 if r == 0 else math.inf for r in raw)
    return tuple(float(r) / scale for r in raw)


# ---------------------------------------------------------------- inputs
GRID = 4096.0


def _grid(t):
    return (torch.round(t * GRID) / GRID).float()


@torch.no_grad()
def frozen_outputs(cfg, sd, obs, spatial, bert=False):
    """(rgb_features, depth_features, BERT stream or None) of one model's frozen parts: the computation of tests/features_ref.trunk_features and
    oracle/hcm_oracle.bert_encoder in float64, rounded to multiples of 1 / GRID.  In float32 these depend on the machine -- with 8 and with 16
    threads the depth trunk and BERT differ in the sixth digit, which moves every gradient by as much and a ReLU across its kink now and then --
    and a fixture is then only good where it was made.  Float64 runs agree to 1e-13 between thread counts, so a value would have to lie that
    close to a rounding boundary 2.4e-4 wide to come out different: the inputs are the same bits everywhere.  The frozen parts are inputs
    here, not under test: both sides are handed these tensors."""
    w = hcm_oracle.Weights({k: np.asarray(v, np.float64) for k, v in sd.items() if k.startswith(train.HCM_HIGH_FROZEN_PREFIXES)})
    rgb = torch.as_tensor(np.asarray(obs["rgb"])).double().permute(0, 3, 1, 2) / 255.0
    x = hcm_oracle.tv_resnet50_trunk(rgb.contiguous(), w.sub("rgb_encoder.cnn."))
    x = F.adaptive_avg_pool2d(x, (4, 4) if spatial else 1)
    d = hcm_oracle.habitat_resnet_encoder(torch.as_tensor(np.asarray(obs["depth"])).double(), w.sub("depth_encoder.visual_encoder."),
                                          cfg.depth_baseplanes // 2)
    stream = None
    if bert:
        ids = torch.as_tensor(np.asarray(obs["instruction"])).long()
        stream = _grid(hcm_oracle.bert_encoder(ids, w.sub("embedding_layer."), cfg.bert_layers, cfg.bert_heads))
    return _grid(x).contiguous(), _grid(d).contiguous(), stream


def inputs(name):
    return inputs_with(name, SEEDS.get(name, cases.SEED))


@functools.lru_cache(maxsize=None)
def inputs_with(name, seed):
    """Everything one call takes, float32 on the CPU, from the seeds: dict(kind, cfg, T, N, sd {model: state dict}, obs (the observations the
    train modules take: the trunk features of frozen_outputs -- (high, low) pairs for the pair -- the token ids or frozen_outputs' BERT
    stream, the oracle sub-task, progress), ids, masks (rows, 2), prev, corrected, stop, h0).  Computed once."""
    kind, cfg, T, N, _ = case(name)
    rows = T * N
    if kind == "hier":
        hi_sd, lo_sd = synth.materialize(synth.high_level_spec(cfg), "hi", seed), synth.materialize(synth.low_level_spec(cfg), "lo", seed)
        raw, corrected, stop, m = val_ref.observations(cfg, T, N)
        hi_rgb, hi_depth, stream = frozen_outputs(cfg, hi_sd, raw, spatial=True, bert=True)
        lo_rgb, lo_depth, _ = frozen_outputs(cfg, lo_sd, raw, spatial=False)
        ids = torch.as_tensor(np.asarray(raw["instruction"])).long()
        obs = {"rgb_features": (hi_rgb, lo_rgb), "depth_features": (hi_depth, lo_depth), "instruction_features": stream,
               "vln_oracle_action_sensor": torch.from_numpy(raw["vln_oracle_action_sensor"])}
        sd, h0 = {"hi": hi_sd, "lo": lo_sd}, val_ref.h0(cfg, N)
    else:
        sd = {"net": synth.make_cma_weights(cfg, seed) if kind == "cma" else synth.make_s2s_weights(cfg, seed)}
        raw = fv.observations(kind, cfg, T, N)
        corrected, stop = fv.labels(T, N)
        m, h0 = fv.masks(kind, T, N), fv.h0(kind, cfg, N)
        rgb, depth, _ = frozen_outputs(cfg, sd["net"], raw, spatial=kind == "cma")
        ids = torch.as_tensor(np.asarray(raw["instruction"])).long()
        obs = {"rgb_features": rgb, "depth_features": depth, "instruction": ids}
        if "progress" in raw:
            obs["progress"] = torch.from_numpy(raw["progress"])
    masks = torch.from_numpy(np.asarray(m, np.float32)).view(rows, 1).expand(rows, 2).contiguous()
    return dict(kind=kind, cfg=cfg, T=T, N=N, sd=sd, obs=obs, ids=ids, masks=masks, prev=torch.zeros(rows, 2), corrected=torch.from_numpy(corrected),
                stop=torch.from_numpy(stop), h0=h0)


def trajectory_inputs(name):
    """inputs(name) cut to the first TRAJECTORY_T[name] steps of the chunk (time-major rows: the first T * N); the whole chunk without an entry"""
    c = inputs(name)
    T = TRAJECTORY_T.get(name, c["T"])
    if T == c["T"]:
        return c
    rows = T * c["N"]

    def cut(v):
        return tuple(t[:rows] for t in v) if isinstance(v, tuple) else v[:rows]
    out = dict(c, T=T, obs={k: cut(v) for k, v in c["obs"].items()})
    out.update({k: c[k][:rows] for k in ("ids", "masks", "prev", "corrected", "stop")})
    return out


def convert_obs(obs, conv):
    """the observations with every floating tensor (the pairs' entries too) through conv and the token ids moved only"""
    probe = conv(torch.zeros(1))

    def one(t):
        return conv(t) if t.dtype.is_floating_point else t.to(probe.device)
    return {k: tuple(one(t) for t in v) if isinstance(v, tuple) else one(v) for k, v in obs.items()}


# ---------------------------------------------------------------- the train modules on a case
def modules(name, conv):
    """{model: train module} with the case's weights, in eval mode (dropout is the identity, as in the fixture), through conv"""
    c = inputs(name)
    kind, cfg = c["kind"], c["cfg"]
    if kind == "hier":
        nets = {"hi": train.HighLevel(cfg), "lo": train.LowLevel(cfg)}
    elif kind == "cma":
        nets = {"net": train.CMANet(cfg, progress_monitor=False)}
    else:
        nets = {"net": train.Seq2SeqNet(cfg)}
    for tag, net in nets.items():
        net.load_reference_state_dict(c["sd"][tag])
        nets[tag] = conv(net.eval())
    return nets


def forward_backward(name, nets, conv):
    """One update_loss and backward of every model, as the update steps order them, and the models' raw outputs from a forward of their own.
    -> dict(losses (TERMS,), counts, outputs {name: tensor}, state {model: tensor}); the gradients are left on the parameters."""
    c = inputs(name)
    obs, masks, prev, h0 = convert_obs(c["obs"], conv), conv(c["masks"]), conv(c["prev"]), conv(c["h0"])
    out = dict(outputs={}, state={})
    if c["kind"] == "hier":
        oracle = obs["vln_oracle_action_sensor"]
        sub = val_ref.remap(c["obs"]["vln_oracle_action_sensor"], c["cfg"].num_sub_tasks).to(h0.device)
        res_hi, out["state"]["hi"] = nets["hi"].update_loss((obs, h0.clone(), prev, masks), oracle)
        res_hi[0].backward()
        res_lo, out["state"]["lo"] = nets["lo"].update_loss((obs, h0.clone(), prev, masks, sub), c["corrected"], c["stop"])
        (res_lo[0] + res_lo[1]).backward()
        out["losses"] = torch.stack([res_hi[0], res_lo[0], res_lo[1]]).detach()
        out["counts"] = [float(res_hi.detach()[3]), float(res_hi.detach()[4]), float(res_hi.detach()[6]), float(res_lo.detach()[3])]
        with torch.no_grad():
            out["outputs"]["logits"] = nets["hi"]((obs, h0.clone(), prev, masks))[0]
            out["outputs"]["vel"], out["outputs"]["stop"], _ = nets["lo"]((obs, h0.clone(), prev, masks, sub))
    else:
        res, out["state"]["net"] = nets["net"].update_loss((obs, h0.clone(), prev, masks), c["corrected"], c["stop"])
        (res[0] + res[1] + res[2]).backward()
        out["losses"] = res[:3].detach()
        out["counts"] = [float(res.detach()[3]), float(res.detach()[4])]
        with torch.no_grad():
            out["outputs"]["out"], out["outputs"]["stop"], _ = nets["net"]((obs, h0.clone(), prev, masks))
    return out


def trajectory(name, nets, conv):
    """STEPS update steps on the same chunk with Adam (ADAM) and the state carried -> (losses (STEPS, TERMS), counts of every step,
    {model: final state}); the parameters are left updated"""
    c = trajectory_inputs(name)
    obs, masks, prev = convert_obs(c["obs"], conv), conv(c["masks"]), conv(c["prev"])
    opts = {tag: torch.optim.Adam(net.parameters(), **ADAM) for tag, net in nets.items()}
    state = {tag: conv(c["h0"]).clone() for tag in nets}
    losses, counts = [], []
    for _ in range(STEPS):
        if c["kind"] == "hier":
            res_hi, res_lo, state["hi"], state["lo"] = train.hier_update(nets["hi"], nets["lo"], opts["hi"], opts["lo"], obs, prev, masks,
                                                                         c["corrected"], c["stop"], state["hi"], state["lo"])
            losses.append(torch.stack([res_hi[0], res_lo[0], res_lo[1]]))
            counts.append([float(res_hi[3]), float(res_hi[4]), float(res_hi[6]), float(res_lo[3])])
        else:
            res, state["net"] = train.flat_update(nets["net"], opts["net"], obs, prev, masks, c["corrected"], c["stop"], state["net"])
            losses.append(res[:3])
            counts.append([float(res[3]), float(res[4])])
        assert all(not s.requires_grad for s in state.values())
    return torch.stack(losses), counts, state


@contextlib.contextmanager
def relu_inputs(record):
    """record(x) for every ReLU input of the CPU path: train/models.py and train/ops.py call torch.relu, an nn.ReLU module F.relu"""
    relu, f_relu = torch.relu, F.relu

    def patched(x):
        record(x.detach())
        return relu(x)

    def f_patched(x, inplace=False):
        record(x.detach())
        return f_relu(x, inplace)
    torch.relu, F.relu = patched, f_patched
    try:
        yield
    finally:
        torch.relu, F.relu = relu, f_relu


def kink_margin(name, seed):
    """How far the ReLUs of a case stay from their kink, the single step and every step of the trajectory: over the ReLU calls, the smallest
    ratio of the call's smallest non-zero |pre-activation| in float64 to the largest deviation of the call's float32 pre-activations from their
    float64 values.  An input that is exactly zero stays so in every precision."""
    old = SEEDS.get(name)
    SEEDS[name] = seed
    try:
        inputs(name)                                           # the frozen trunks run here, outside the recording
        seen = {}
        for tag, conv in (("64", lambda t: t.double()), ("32", lambda t: t)):
            seen[tag] = []
            with relu_inputs(lambda x, tag=tag: seen[tag].append(x.double().clone())):
                forward_backward(name, modules(name, conv), conv)
                if name in TRAJECTORY:
                    trajectory(name, modules(name, conv), conv)
        assert len(seen["64"]) == len(seen["32"]) > 0
        ratios = [x[x != 0].abs().min().item() / (y - x).abs().max().item() for x, y in zip(seen["64"], seen["32"]) if (x != 0).any() and not torch.equal(x, y)]
        return float(np.min(ratios))
    finally:
        SEEDS.pop(name)
        if old is not None:
            SEEDS[name] = old


def conditioning(name, seed):
    """the largest per-tensor max|t32 - t64| / max|t64| of the train modules' float32 CPU run against their float64 run with the weights of
    `seed`: the losses, outputs, states and gradients of the single step (a cancelling key bias on its weight's scale) and, for a trajectory
    case, the losses of every step, the final state and every final parameter"""
    old = SEEDS.get(name)
    SEEDS[name] = seed
    try:
        runs = {}
        for tag, conv in (("64", lambda t: t.double()), ("32", lambda t: t)):
            nets = modules(name, conv)
            run = forward_backward(name, nets, conv)
            t = {"losses": run["losses"], **{"out/" + k: v for k, v in run["outputs"].items()}, **{"state/" + k: v for k, v in run["state"].items()}}
            t.update({f"grad/{m}/{k}": p.grad for m, net in nets.items() for k, p in net.named_parameters() if p.grad is not None})
            if name in TRAJECTORY:
                nets = modules(name, conv)
                losses, _, state = trajectory(name, nets, conv)
                t.update({"traj_losses": losses, **{"final state/" + k: v for k, v in state.items()}})
                t.update({f"final/{m}/{k}": p for m, net in nets.items() for k, p in net.named_parameters()})
            runs[tag] = {k: v.detach().double() for k, v in t.items()}
        kind, hh = inputs(name)["kind"], inputs(name)["cfg"].hidden // 2
        worst = []
        for k, ref in runs["64"].items():
            zb = zero_bias(kind, k[5:], hh) if k.startswith("grad/") else None
            scale = runs["64"]["grad/" + zb[0]].abs().max().item() if zb else ref.abs().max().item()
            err = (runs["32"][k] - ref).abs().max().item()
            worst.append(err / scale if scale > 0 else (0.0 if err == 0 else math.inf))
        return worse(*worst)
    finally:
        SEEDS.pop(name)
        if old is not None:
            SEEDS[name] = old


def first_seed(name):
    seed = cases.SEED
    while kink_margin(name, seed) < KINK_RATIO or conditioning(name, seed) > SEED_BOUND:
        seed += 1
    return seed


# ---------------------------------------------------------------- the fixture
def load(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def partition(gold):
    """the fixture's sets of state-dict keys ("model/key"): parameters with a gradient (a `grad/<key>` entry each), with None, frozen ones,
    and the buffers (the string lists `nograd`, `frozen`, `buffer`: an entry per key would cost the file a third of its size limit)"""
    return ({k.split("/", 1)[1] for k in gold if k.startswith("grad/")},) + tuple(set(gold[p].tolist()) for p in ("nograd", "frozen", "buffer"))


def zero_bias(kind, key, hh):
    """A key bias cancels in the softmax, so its exact gradient is zero: (partner weight's key, the slice of the bias it covers, whether the
    train module promises exact zeros) or None.  CMANet's text_k.bias goes through _ZeroGrad and the key halves of rgb_kv / depth_kv take
    no part in its forward: exact zeros; the cross-modal encoder's fc_k.bias gets what the kernels and float arithmetic leave."""
    if kind == "cma" and key in ("net/text_k.bias", "net/rgb_kv.bias", "net/depth_kv.bias"):
        return key[:-4] + "weight", slice(None) if key == "net/text_k.bias" else slice(0, hh), True
    if kind == "hier" and key.endswith("enc_att.attention.fc_k.bias"):
        return key[:-4] + "weight", slice(None), False
    return None


def compare(name, gold, nets, run, traj, what):
    """Every figure of a run (forward_backward's dict) and, where the fixture has one, of a trajectory against the fixture -> {label: error as a
    multiple of the reference's scale}.  Also asserts what is exact: the partition, the counts, the promised zeros."""
    c = inputs(name)
    kind, sub = c["kind"], int(gold["subsample"])
    worst = {}

    def rel(label, got, ref):
        got, ref = np.asarray(got.detach().cpu().double().numpy() if torch.is_tensor(got) else got, np.float64), np.asarray(ref, np.float64)
        assert got.shape == ref.shape, (label, got.shape, ref.shape)
        worst[label] = float(np.abs(got - ref).max() / np.abs(ref).max())

    if run is not None:
        for k in range(TERMS):
            if gold["losses"][k] != 0:
                rel(f"loss[{k}]", run["losses"][k:k + 1], gold["losses"][k:k + 1])
            else:
                assert float(run["losses"][k]) == 0.0, k                    # no progress monitor: the aux term is an exact 0
        assert run["counts"] == gold["counts"].tolist(), (run["counts"], gold["counts"])
        for key, t in run["outputs"].items():
            rel("out/" + key, t, gold["out/" + key])
        for tag, t in run["state"].items():
            rel("state/" + tag, t, gold["state/" + tag])
        grad, nograd, frozen, buffers = partition(gold)
        ours_grad, ours_none = set(), set()
        for tag, net in nets.items():
            outside = {k for k in grad | nograd | frozen | buffers if k.startswith(tag + "/") and not k.split("/", 1)[1].startswith(FROZEN[tag])}
            assert {f"{tag}/{k}" for k in net.state_dict()} == outside, tag
            assert not outside & frozen, tag                                # outside the frozen parts every parameter trains
            for k, p in net.named_parameters():
                (ours_none if p.grad is None else ours_grad).add(f"{tag}/{k}")
        # the frozen BERT keeps requires_grad and runs under no_grad: None there, as everything inside the frozen parts is frozen or None
        inside = {k for k in nograd if k.split("/", 1)[1].startswith(FROZEN[k.split("/", 1)[0]])}
        assert ours_grad == grad, (sorted(ours_grad - grad), sorted(grad - ours_grad))
        assert ours_none == nograd - inside, (sorted(ours_none - nograd), sorted(nograd - inside - ours_none))
        hh = c["cfg"].hidden // 2
        for tag, net in nets.items():
            for k, p in net.named_parameters():
                key = f"{tag}/{k}"
                if p.grad is None:
                    continue
                g = p.grad.detach().cpu().double().numpy()
                zb = zero_bias(kind, key, hh)
                if zb is None:
                    e = errors(key, g, gold["grad/" + key], gold["gstat/" + key], gold["gproj/" + key], sub)
                    worst["grad/" + key], worst["gsum/" + key], worst["gproj/" + key] = worse(e[0], e[1]), e[2], e[3]
                    continue
                partner, where, exact = zb
                scale = float(gold["gstat/" + partner][0])
                ref, flat = gold["grad/" + key], g.reshape(-1)
                pos = np.arange(0, flat.size, stride_of(flat.size, sub))    # the stored positions
                zero = np.zeros(flat.size, bool)
                zero[where] = True
                assert ref.shape == pos.shape and zero[pos].any(), key
                assert np.abs(ref[zero[pos]]).max() <= 1e-12 * scale, key   # the reference itself: zero up to float64 noise
                if exact:
                    assert (flat[zero] == 0).all(), key
                else:
                    worst["grad/" + key + " (on its weight's scale)"] = float(np.abs(flat[pos][zero[pos]] - ref[zero[pos]]).max() / scale)
                if not zero.all():                                          # the value half of a kv bias: by the rule of every other tensor
                    worst["grad/" + key + " (value half)"] = float(np.abs(flat[pos][~zero[pos]] - ref[~zero[pos]]).max() / gold["gstat/" + key][0])
    if traj is not None:
        losses, counts, state = traj
        for s in range(STEPS):
            for k in range(TERMS):
                if gold["traj_losses"][s, k] != 0:
                    rel(f"step {s} loss[{k}]", losses[s, k:k + 1], gold["traj_losses"][s, k:k + 1])
                else:
                    assert float(losses[s, k]) == 0.0
            assert counts[s] == gold["traj_counts"][s].tolist(), s
        for tag, t in state.items():
            rel("final state/" + tag, t, gold["traj_state/" + tag])
        for tag, net in nets.items():
            for k, p in net.named_parameters():
                key = f"{tag}/{k}"
                e = errors("final/" + key, p.detach().cpu().double().numpy(), gold["final/" + key], gold["fstat/" + key], gold["fproj/" + key], sub)
                worst["final/" + key], worst["fsum/" + key], worst["fproj/" + key] = worse(e[0], e[1]), e[2], e[3]
    top = max(worst, key=lambda k: math.inf if math.isnan(worst[k]) else worst[k])
    print(f"{name} {what}: worst {worst[top]:.3e} ({top}); losses {worse(*(v for k, v in worst.items() if 'loss' in k)):.3e}, "
          f"gradients {worse(*(v for k, v in worst.items() if k.startswith('g'))):.3e}, "
          f"final parameters {worse(*(v for k, v in worst.items() if k.startswith('f'))):.3e}")
    return worst
