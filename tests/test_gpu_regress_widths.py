"""-m gpu: the MLP regression step at widths without a tuned tile (GradMlpGen + the run-time-width reduce kernel,
csrc/ionode_grad_gen.hpp), against torch on the CPU, against the tuned kernels where both serve a width, and end to end.

Tolerances are tests/test_regression.py:22's (LOSS_RTOL, GRAD_RTOL, FIT_RTOL = 2e-6, 2e-4, 2e-3: the GPU sums the squared residuals
per workgroup in fp64 and the weight gradient on the fp32 MFMA in another order than torch's CPU kernels).  The inputs are
test_other_architectures_against_torch's recipe with M = 1003 rows (63 tiles, the last with 11 valid rows); on those seeds torch fp32
against torch fp64 stays within 7.5e-8 (loss), 2.8e-7 (gradient rel-L2) and 2.8e-5 (five-step loss curve), so the bounds have >= 25x /
700x / 70x of room."""
import importlib
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

import kat_cases as K

pytestmark = pytest.mark.gpu

LOSS_RTOL, GRAD_RTOL, FIT_RTOL = 2e-6, 2e-4, 2e-3   # tests/test_regression.py:22
M_ROWS = 1003


def _reg():
    return importlib.import_module("neural-ode-ion-channels_amd.regression")


def _case(L, N, with_offset):
    rng = np.random.default_rng(L * 1000 + N)
    M = M_ROWS
    x = np.stack([rng.uniform(-1.3, 0.7, M), rng.uniform(0.01, 0.99, M)], 1).astype(np.float32)
    y = rng.normal(0, 1e-3, M).astype(np.float32)
    off = rng.normal(0, 1e-3, M).astype(np.float32) if with_offset else None
    parts = []
    for (o, i) in [(N, 2)] + [(N, N)] * L + [(1, N)]:
        parts += [rng.normal(0, 0.3, o * i).astype(np.float32), rng.normal(0, 0.1, o).astype(np.float32)]
    return x, y, off, np.concatenate(parts)


def _net(w, L, N):
    layers = [nn.Linear(2, N), nn.LeakyReLU()]
    for _ in range(L):
        layers += [nn.Linear(N, N), nn.LeakyReLU()]
    net = nn.Sequential(*layers, nn.Linear(N, 1))
    o = 0
    with torch.no_grad():
        for m in net:
            if isinstance(m, nn.Linear):
                n = m.weight.numel()
                m.weight.copy_(torch.from_numpy(w[o:o + n].reshape(m.weight.shape))); o += n
                m.bias.copy_(torch.from_numpy(w[o:o + m.bias.numel()])); o += m.bias.numel()
    return net


def _flat(net):
    return np.concatenate([np.concatenate([m.weight.detach().numpy().ravel(), m.bias.detach().numpy().ravel()])
                           for m in net if isinstance(m, nn.Linear)])


def _torch_loss(net, x, y, offset=None):
    p = net(torch.from_numpy(x)) / 1000.0
    if offset is not None:
        p = p + torch.from_numpy(offset).reshape(-1, 1)
    return nn.MSELoss(reduction="sum")(p.reshape(-1), torch.from_numpy(y))


# F = 0 with R = 2 (17) at one and at fifteen layers (every sign word), R = 0 and exact multiples of 16 (64), R = 2 with F = 2 (150),
# R = 3 (50: F = 0; 300: F = 4), F = 7 with R = 1 (464: two reduce row blocks, the widest tile the LDS takes)
@pytest.mark.parametrize("L,N,with_offset", [(1, 17, False), (15, 17, True), (2, 50, True), (5, 64, False), (3, 150, False),
                                             (2, 300, True), (5, 300, False), (1, 464, False), (2, 464, False)])
def test_loss_gradient_and_adam_steps_against_torch(ion, gpu, monkeypatch, L, N, with_offset):
    monkeypatch.delenv("IONODE_GRAD_GENERIC", raising=False)
    assert ion.capi.regress_plan(L, N)["generic"]
    x, y, off, w = _case(L, N, with_offset)
    r = _reg().MlpRegression(w, L, N, x, y, off, device=gpu)
    loss, g = r.loss_and_grad()
    assert g.shape == (2 * N + N + L * (N * N + N) + N + 1,)          # flat state-dict order: no padding entries
    net = _net(w, L, N)
    ref = _torch_loss(net, x, y, off)
    ref.backward()
    gref = np.concatenate([np.concatenate([m.weight.grad.numpy().ravel(), m.bias.grad.numpy().ravel()])
                           for m in net if isinstance(m, nn.Linear)])
    el = abs(loss.item() - ref.item()) / ref.item()
    eg = float(np.linalg.norm(g.cpu().numpy() - gref) / np.linalg.norm(gref))
    print(f"(L={L}, N={N}): loss rel {el:.2e}, grad rel-L2 {eg:.2e}")
    assert el <= LOSS_RTOL and eg <= GRAD_RTOL
    net = _net(w, L, N)
    opt = torch.optim.Adam(net.parameters(), lr=0.001)
    for _ in range(5):
        l_t = _torch_loss(net, x, y, off)
        opt.zero_grad(); l_t.backward(); opt.step()
        l_g = r.step()
        assert abs(l_g.item() - l_t.item()) <= FIT_RTOL * l_t.item()
    assert np.linalg.norm(r.state_dict_flat() - _flat(net)) / np.linalg.norm(_flat(net)) <= FIT_RTOL


@pytest.mark.parametrize("L,N", [(5, 10), (3, 100), (5, 200), (1, 500)])
def test_records_equal_the_tuned_kernels_bit_for_bit(ion, gpu, monkeypatch, L, N):
    """Canonical order: at the widths both serve, GradMlpGen's forward recompute, seeds and gradient tiles are the tuned GradMlp's bits --
    the whole record buffer and the loss.  The weight gradients (same slab count, the two reduce kernels) agree to GRAD_RTOL; whether
    they are bit-equal too is printed, not asserted (on an MI355X they were, at all four shapes: both kernels run the same chains)."""
    monkeypatch.setenv("IONODE_REGRESS_WG_PER_CU", "1")
    x, y, off, w = _case(L, N, N == 100)
    monkeypatch.delenv("IONODE_GRAD_GENERIC", raising=False)
    n_slabs = int(ion.capi.lib().ionode_grad_reduce_slabs(L, N, (M_ROWS + 15) // 16))
    monkeypatch.setenv("IONODE_REGRESS_SLABS", str(n_slabs))
    got = {}
    for tag in ("tuned", "generic"):
        if tag == "generic":
            monkeypatch.setenv("IONODE_GRAD_GENERIC", "1")
        assert ion.capi.regress_plan(L, N)["generic"] == (tag == "generic")
        r = _reg().MlpRegression(w, L, N, x, y, off, device=gpu)
        assert r.n_slabs == n_slabs
        r.records.zero_()
        loss, g = r.loss_and_grad()   # _forward_backward() once, then the slab sum
        got[tag] = (r.records.clone(), r.loss_part.clone(), g.clone())
    assert torch.equal(got["tuned"][0], got["generic"][0])
    assert torch.equal(got["tuned"][1], got["generic"][1])
    gt, gg = got["tuned"][2].double(), got["generic"][2].double()
    print(f"(L={L}, N={N}): gradients bit-equal: {torch.equal(got['tuned'][2], got['generic'][2])}, rel-L2 {float((gg - gt).norm() / gt.norm()):.2e}")
    assert float((gg - gt).norm() / gt.norm()) <= GRAD_RTOL


def test_unit_seed_reduce_through_the_solve(ion, gpu, monkeypatch):
    """grad.solve at N = 100 (tuned sweep kernels either way) with the run-time-width reduce kernel scaling the unit-seed records while it
    stages them: dL/dW within 1e-5 of the tuned reduce (include/ionode.h's bound for reorderings of the fp32 product: the slab
    count is each kernel's own and may differ), dL/dp and dL/dy0 identical (the reduce does not touch them).  B = 20: a ragged second tile."""
    grad = importlib.import_module("neural-ode-ion-channels_amd.grad")
    capi = ion.capi
    L, N, B, Nt = 2, 100, 20, 2001
    P = ion.protocols
    pv = P.sinewave(P.sinewave_scales(0, B), n_samples=Nt, xp=torch, device=gpu)
    te = torch.arange(0, 1200, 4, dtype=torch.float64, device=gpu) * 0.1     # 300 output samples
    w0 = np.random.default_rng(N).normal(0, 0.1, 2 * N + N + L * (N * N + N) + N + 1).astype(np.float32)
    got = {}
    for tag in ("tuned", "generic"):
        if tag == "generic":
            monkeypatch.setenv("IONODE_GRAD_GENERIC", "1")
        else:
            monkeypatch.delenv("IONODE_GRAD_GENERIC", raising=False)
        w = torch.from_numpy(w0.copy()).to(gpu).requires_grad_(True)
        params = torch.from_numpy(np.tile(K.P_HH, (B, 1)) * np.random.default_rng(5).uniform(0.9, 1.1, (B, 8))).to(gpu).requires_grad_(True)
        y0 = torch.tensor([[0.0, 1.0]], dtype=torch.float32, device=gpu).repeat(B, 1).requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            y, status = grad.solve(capi.MODEL_NNF, w, params, pv, y0, te, mlp_layers=L, mlp_width=N, prot_t0=0.0, prot_dt=0.1)
        assert bool((status == 0).all())
        (y[..., 0] * y[..., 1]).double().sum().backward()
        got[tag] = (w.grad.clone(), params.grad.clone(), y0.grad.clone())
    a, b = got["generic"][0].double(), got["tuned"][0].double()
    assert float(b.norm()) > 0
    rel = float((a - b).norm() / b.norm())
    print(f"unit-seed reduce: dL/dW rel-L2 {rel:.2e}")
    assert rel <= 1e-5
    assert torch.equal(got["generic"][1], got["tuned"][1]) and torch.equal(got["generic"][2], got["tuned"][2])


def test_train_a_64_wide_net_then_predict_with_it(ion, gpu, oracle, monkeypatch):
    """What the feature is for: a width the package could integrate but not fit.  Rows (V / 100, a) -> da/dt of the HH 2-state model
    (kat_cases.P_HH) along three activation steps; 300 iterations of the reference loop; the loss falls by > 20x (the criterion of
    tests/test_gpu_end_to_end.py); the trained weights then drive the forward solve, bit-identical to the CPU oracle."""
    monkeypatch.delenv("IONODE_GRAD_GENERIC", raising=False)
    L, N = 2, 64
    p = K.P_HH
    steps = (-40, 0, 40)
    xs, ys, pvs = [], [], []
    for v in steps:
        tp, pv, te = K.activation(v)
        tr = te[::8]
        a = oracle.solve(K.MODEL_HH2, p, pv, [0.0, 1.0], tr, prot_t0=0.0, prot_dt=1.0)["y"][0, :, 0]
        V = np.interp(tr, tp, pv)
        xs.append(np.stack([V / 100.0, a], 1))
        ys.append(p[0] * np.exp(p[1] * V) * (1.0 - a) - p[2] * np.exp(-p[3] * V) * a)
        pvs.append(pv)
    x, y = np.concatenate(xs).astype(np.float32), np.concatenate(ys).astype(np.float32)
    rng = np.random.default_rng(64)
    parts = []
    for (o, i) in [(N, 2)] + [(N, N)] * L + [(1, N)]:          # the reference's initialisation: N(0, 0.1^2), zero bias
        parts += [rng.normal(0, 0.1, o * i).astype(np.float32), np.zeros(o, dtype=np.float32)]
    w0 = np.concatenate(parts)
    r = _reg().MlpRegression(w0, L, N, x, y, lr=1e-3, step_size=100, gamma=0.9, device=gpu)
    first = float(r.loss_and_grad()[0].item())
    r.fit(300)
    last = float(r.loss_and_grad()[0].item())
    print(f"N = 64 fit: loss {first:.3e} -> {last:.3e}")
    assert last < first / 20.0, (first, last)
    w = r.state_dict_flat()
    pv = np.stack(pvs)
    te = K.activation(0)[2][::16]                               # 501 output samples
    pot = np.arange(3, dtype=np.int32)
    params = np.tile(p, (3, 1))
    sol = ion.solve(K.MODEL_NNF, params, pv, torch.tensor([[0.0, 1.0]], dtype=torch.float64), te, weights=w, mlp_layers=L, mlp_width=N,
                    prot_t0=0.0, prot_dt=1.0, prot_of_traj=pot, device=gpu)
    o = oracle.solve(K.MODEL_NNF, params, pv, [0.0, 1.0], te, weights=w, mlp_layers=L, mlp_width=N, prot_t0=0.0, prot_dt=1.0, prot_of_traj=pot)
    assert np.array_equal(sol.status.cpu().numpy(), o["status"]) and (o["status"] == 0).all()
    assert np.array_equal(sol.y.cpu().numpy(), o["y"])


@pytest.mark.parametrize("L,N,text", [(1, 490, "LDS"), (16, 64, "outside the served shapes")])
def test_unserved_shapes_raise_before_anything_is_allocated(ion, gpu, monkeypatch, L, N, text):
    monkeypatch.delenv("IONODE_GRAD_GENERIC", raising=False)
    n = 2 * N + N + L * (N * N + N) + N + 1
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    with pytest.raises(ion.capi.IonodeError, match=text) as e:
        _reg().MlpRegression(np.zeros(n, dtype=np.float32), L, N, np.zeros((32, 2), np.float32), np.zeros(32, np.float32), device=gpu)
    assert "ionode_regress_step" in str(e.value)                # the library's text
    assert torch.cuda.memory_allocated(gpu) == before
    # ... and the C entry point itself launches nothing for such a shape (it refuses before it looks at a pointer's target)
    buf = torch.zeros(64, dtype=torch.float32, device=gpu)
    pp = lambda: __import__("ctypes").c_void_p(buf.data_ptr())
    rc = ion.capi.lib().ionode_regress_step(L, N, pp(), pp(), None, pp(), 32, __import__("ctypes").c_float(1000.0), pp(), pp(), 1, None)
    assert rc == -2
    torch.cuda.synchronize()
