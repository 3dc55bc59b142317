"""The differentiable state encoder without a GPU: the two C ABI symbols (declaration, binding, argument checks in front of every device
call) and robo_vln_amd.train's module surface and CPU restatement (against torch's cells, and its gradients by gradcheck)."""
import ctypes as C
import os
import re

import pytest
import torch

from robo_vln_amd import _lib, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM, GRU = _lib.HCM_LSTM, _lib.HCM_GRU
# The positive controls hand host buffers to a fully valid call and expect HCM_ERR_HIP from the missing device.  Where a device is visible the
# same call would launch kernels on host pointers, so the controls run only without one; the -1 cases never reach a launch anywhere.
NO_DEVICE = not torch.cuda.is_available()


def test_header_declares_and_binding_agrees():
    text = open(os.path.join(ROOT, "include", "hcm.h")).read()
    for sym, n in (("hcm_op_state_scan_train", 15), ("hcm_op_state_scan_bwd", 16)):
        m = re.search(r"int %s\(([^;]*)\);" % sym, text)
        assert m, f"include/hcm.h does not declare {sym}"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        res, args = _lib.EXPORTS[sym]
        assert res is C.c_int and len(args) == n_args == n, sym
        assert hasattr(_lib.lib(), sym)


def _p():
    buf = (C.c_float * 64)()
    return C.cast(buf, C.c_void_p)


def test_train_forward_argument_errors_without_a_device():
    l, p = _lib.lib(), _p()

    def call(pre=p, w_hh=p, b_hh=None, h_in=p, masks=p, seq=p, h_out=p, gates=p, c_seq=p, work=p, T=2, N=2, H=512, rnn=LSTM):
        return l.hcm_op_state_scan_train(pre, w_hh, b_hh, h_in, masks, seq, h_out, gates, c_seq, work, T, N, H, rnn, None)

    if NO_DEVICE:
        assert call() == -5 and call(rnn=GRU, c_seq=None, b_hh=p) == -5        # valid arguments: only the missing device stops them
    for name in ("pre", "w_hh", "h_in", "masks", "seq", "h_out", "gates", "work"):
        assert call(**{name: None}) == -1, name
    assert call(T=0) == -1 and call(N=0) == -1 and call(T=-1) == -1
    assert call(H=500) == -1
    assert call(rnn=2) == -1 and call(rnn=-1) == -1
    assert call(rnn=GRU, c_seq=p) == -1                      # c_seq must be NULL for GRU
    assert call(rnn=LSTM, c_seq=None) == -1                  # ... and present for LSTM


def test_backward_argument_errors_without_a_device():
    """`work` is a buffer of its own, so every -1 below comes from the check it names; the positive control (a fully valid call) gets past
    all of them and fails at the device, HCM_ERR_HIP."""
    l, p = _lib.lib(), _p()
    H, N = 512, 2
    big = (C.c_float * (4 * H * H + 4 * N * H + 16))()
    at = lambda i: C.c_void_p(C.addressof(big) + 4 * i)
    wk = at(0)

    def call(d_seq=p, gates=p, c_seq=p, seq=p, h_in=p, masks=p, w_hh=p, work=wk, d_pre=p, d_gh=None, d_h_in=p, T=2, N=N, H=H, rnn=LSTM):
        return l.hcm_op_state_scan_bwd(d_seq, gates, c_seq, seq, h_in, masks, w_hh, work, d_pre, d_gh, d_h_in, T, N, H, rnn, None)

    if NO_DEVICE:
        assert call() == -5 and call(rnn=GRU, c_seq=None, d_gh=p) == -5         # valid arguments: only the missing device stops them
    for name in ("d_seq", "gates", "seq", "h_in", "masks", "w_hh", "work", "d_pre", "d_h_in"):
        assert call(**{name: None}) == -1, name
    assert call(T=0) == -1 and call(N=0) == -1 and call(N=-3) == -1
    assert call(H=500) == -1
    assert call(rnn=2) == -1
    assert call(rnn=GRU, c_seq=p, d_gh=p) == -1 and call(rnn=LSTM, c_seq=None) == -1
    assert call(rnn=LSTM, d_gh=p) == -1 and call(rnn=GRU, c_seq=None, d_gh=None) == -1
    # an output inside `work` (4*H*H packed weights, then the 4*N*H carry floats) would race with the carries
    for name in ("d_h_in", "d_pre"):
        assert call(**{name: at(4 * H * H)}) == -1, name                       # the first carry pair
        assert call(**{name: at(4 * H * H + 4 * N * H - 1)}) == -1, name       # the last float of the second
    assert call(rnn=GRU, c_seq=None, d_gh=at(5)) == -1
    assert call(work=at(16), d_h_in=at(0)) == -1                               # starts in front of it, ends inside
    if NO_DEVICE:
        assert call(d_h_in=at(4 * H * H + 4 * N * H)) == -5                    # the first float behind it: no overlap


@pytest.mark.parametrize("rnn", ["LSTM", "GRU"])
def test_state_dict_is_the_reference_layout(rnn):
    H, I, G = 512, 640, 4 if rnn == "LSTM" else 3
    enc = train.RNNStateEncoder(I, H, rnn_type=rnn)
    sd = enc.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {"rnn.weight_ih_l0": (G * H, I), "rnn.weight_hh_l0": (G * H, H),
                                                          "rnn.bias_ih_l0": (G * H,), "rnn.bias_hh_l0": (G * H,)}
    assert enc.num_recurrent_layers == (2 if rnn == "LSTM" else 1)
    assert sd["rnn.bias_ih_l0"].abs().max() == 0 and sd["rnn.bias_hh_l0"].abs().max() == 0
    w = sd["rnn.weight_hh_l0"]
    assert torch.allclose(w.t() @ w, torch.eye(H), atol=1e-4)                          # orthogonal initialisation
    ref = getattr(torch.nn, rnn)(I, H)                                                 # a reference checkpoint's keys load unchanged
    enc.load_state_dict({"rnn." + k: v for k, v in ref.state_dict().items()})
    assert torch.equal(enc.rnn.weight_hh_l0, ref.weight_hh_l0)


def _randomise(mod, g, scale=0.2):
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_((torch.rand(p.shape, generator=g, dtype=p.dtype) - 0.5) * scale)


def _masks(T, N, g):
    m = (torch.rand(T, N, generator=g) > 0.4).float()
    m[0, 0] = 0
    if T > 2:
        m[T // 2, N // 2] = 0
    m[T - 1, N - 1] = 0
    return m


@pytest.mark.parametrize("rnn", ["LSTM", "GRU"])
def test_cpu_path_equals_torch_cells(rnn):
    H, I, T, N = 512, 32, 5, 3
    g = torch.Generator().manual_seed(7)
    enc = train.RNNStateEncoder(I, H, rnn_type=rnn)
    _randomise(enc, g)
    cell = (torch.nn.LSTMCell if rnn == "LSTM" else torch.nn.GRUCell)(I, H)
    cell.load_state_dict({k[4:-3]: v for k, v in enc.state_dict().items()})
    x = torch.rand(T * N, I, generator=g) * 2 - 1
    h0 = torch.rand(enc.num_recurrent_layers, N, H, generator=g) - 0.5
    m = _masks(T, N, g)
    with torch.no_grad():
        h, c = h0[0], (h0[1] if rnn == "LSTM" else None)
        ref = []
        for t in range(T):
            mk = m[t].view(N, 1)
            if rnn == "LSTM":
                h, c = cell(x[t * N:(t + 1) * N], (h * mk, c * mk))
            else:
                h = cell(x[t * N:(t + 1) * N], h * mk)
            ref.append(h)
        ref_seq, ref_h = torch.cat(ref, 0), (torch.stack([h, c], 0) if rnn == "LSTM" else h[None])
        for masks in (m.reshape(-1), m.reshape(-1, 1)):
            seq, hid = enc(x, h0, masks)
            e_s, e_h = (seq - ref_seq).abs().max().item(), (hid - ref_h).abs().max().item()
            print(f"cpu path [{rnn}]: seq {e_s:.3e} hidden {e_h:.3e}")
            assert seq.shape == (T * N, H) and hid.shape == h0.shape and e_s <= 1e-6 and e_h <= 1e-6
        one, hid1 = enc.single_forward(x[:N], h0, m[0].view(N, 1))
        assert (one - ref_seq[:N]).abs().max().item() <= 1e-6 and hid1.shape == h0.shape


@pytest.mark.parametrize("rnn", ["LSTM", "GRU"])
def test_cpu_path_gradcheck(rnn):
    H, I, T, N = 64, 5, 3, 2
    g = torch.Generator().manual_seed(11)
    enc = train.RNNStateEncoder(I, H, rnn_type=rnn).double()
    _randomise(enc, g, 1.0)
    params = [p for p in enc.parameters()]
    names = [n for n, _ in enc.named_parameters()]
    x = (torch.rand(T * N, I, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_()
    h0 = (torch.rand(enc.num_recurrent_layers, N, H, generator=g, dtype=torch.float64) - 0.5).requires_grad_()
    m = torch.tensor([[0., 1.], [1., 1.], [1., 0.]], dtype=torch.float64)

    def fn(x_, h0_, *ps):
        byname = dict(zip(names, ps))
        lp = [tuple(byname[f"rnn.{n}_l0"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))]
        return train.cell_loop(x_, lp, h0_, m.reshape(-1), rnn)[0]

    assert torch.autograd.gradcheck(fn, (x, h0, *params), eps=1e-6, atol=1e-6, rtol=1e-4)


def test_forward_dispatches_by_row_count(monkeypatch):
    enc = train.RNNStateEncoder(8, 16)
    calls = []
    monkeypatch.setattr(enc, "single_forward", lambda *a: calls.append("single") or "s")
    monkeypatch.setattr(enc, "seq_forward", lambda *a: calls.append("seq") or "q")
    h0 = torch.zeros(1, 3, 16)
    assert enc(torch.zeros(3, 8), h0, torch.ones(3, 1)) == "s"
    assert enc(torch.zeros(12, 8), h0, torch.ones(12)) == "q"
    assert calls == ["single", "seq"]


def test_cpu_restatement_serves_other_sizes_and_layers():
    enc = train.RNNStateEncoder(8, 24, num_layers=2, rnn_type="LSTM")
    assert enc.num_recurrent_layers == 4
    g = torch.Generator().manual_seed(3)
    x, h0, m = torch.rand(6, 8, generator=g), torch.rand(4, 2, 24, generator=g), torch.ones(6)
    with torch.no_grad():
        seq, hid = enc(x, h0, m)
        ref, (hn, cn) = enc.rnn(x.view(3, 2, 8), (h0[:2].contiguous(), h0[2:].contiguous()))     # all masks 1: torch's own sequence call
    assert (seq - ref.reshape(6, 24)).abs().max().item() <= 1e-6 and (hid - torch.cat([hn, cn], 0)).abs().max().item() <= 1e-6
