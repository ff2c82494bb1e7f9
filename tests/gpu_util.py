"""Helpers shared by the -m gpu parity tests: run the same inputs through libionode (HIP) and the oracle."""
import numpy as np
import torch


def run_gpu(ion, dev, model, params, prot_v, y0, t_eval, *, weights=None, L=0, N=0, f32=False, **kw):
    capi = ion.capi
    params = np.atleast_2d(np.asarray(params, dtype=np.float64))
    B = params.shape[0]
    prot_v = np.atleast_2d(np.asarray(prot_v, dtype=np.float64))
    y0 = np.broadcast_to(np.atleast_2d(np.asarray(y0, dtype=np.float64)), (B, np.atleast_2d(y0).shape[-1]))
    sdt = torch.float32 if f32 else torch.float64
    packed = None
    if weights is not None:
        packed = torch.from_numpy(capi.mlp_pack(weights, L, N)).to(dev)
    kw.setdefault("t_eval_hint", "auto")
    pt = kw.pop("prot_t", None)
    pot = kw.pop("prot_of_traj", None)
    r = capi.dopri5(
        model,
        torch.from_numpy(np.ascontiguousarray(params)).to(dev),
        torch.from_numpy(np.ascontiguousarray(prot_v)).to(dev),
        torch.from_numpy(np.ascontiguousarray(y0)).to(dev).to(sdt).contiguous(),
        torch.from_numpy(np.ascontiguousarray(np.asarray(t_eval, dtype=np.float64))).to(dev),
        mlp_packed=packed, mlp_layers=L, mlp_width=N,
        prot_t=None if pt is None else torch.from_numpy(np.ascontiguousarray(np.asarray(pt, dtype=np.float64))).to(dev),
        prot_of_traj=None if pot is None else torch.from_numpy(np.ascontiguousarray(np.asarray(pot, dtype=np.int32))).to(dev),
        **kw)
    torch.cuda.synchronize()
    return {"y": r["y"].double().cpu().numpy(), "i": None if r["i"] is None else r["i"].cpu().numpy(),
            "status": r["status"].cpu().numpy(), "stats": r["stats"].cpu().numpy()}


def rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ---- the test-only probe of the device primitives (tests/csrc/ionode_probe.hip -> libionode_probe.so, built by csrc/Makefile) ----
PROBE_OPS = {"det_exp": 0, "det_exp_ldexp": 1, "det_exp_inrange": 2, "det_exp_s": 3, "det_expf": 4, "det_root5": 5, "div_by": 6,
             "div_pos": 7, "div_const_100": 8, "div_constf_1000": 9, "lrelu": 10, "group8_sum_f64": 11, "mbcnt": 12, "compose_cost": 13}
_PROBE_F32 = ("det_expf", "div_constf_1000", "lrelu")
_probe_lib = None


def probe_lib(ion):
    """libionode_probe.so beside libionode.so.  A missing file is an error (the build entry point makes both), never a skip."""
    global _probe_lib
    if _probe_lib is None:
        import ctypes as C
        import os
        # IONODE_PROBE_LIB: dev override, as IONODE_LIB is for libionode.so (a mutated build of the headers under test)
        path = os.environ.get("IONODE_PROBE_LIB") or os.path.join(os.path.dirname(os.path.abspath(ion.capi.__file__)), "libionode_probe.so")
        if not os.path.exists(path):
            raise ion.capi.IonodeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(path)
        L.ionode_probe.restype = C.c_int
        L.ionode_probe.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_longlong, C.c_void_p]
        L.ionode_probe_div_constf_sweep.restype = C.c_int
        L.ionode_probe_div_constf_sweep.argtypes = [C.c_void_p, C.c_void_p]
        _probe_lib = L
    return _probe_lib


def probe(ion, dev, op, a, b=None, c=None):
    """op over numpy arrays on the device: float64 in and out, float32 for det_expf / div_constf_1000 / lrelu, uint64 masks (and an
    optional int32 b) -> int32 for mbcnt.  Returns a numpy array of a's shape."""
    L = probe_lib(ion)
    in_dt = np.float32 if op in _PROBE_F32 else (np.uint64 if op == "mbcnt" else np.float64)
    out_dt = torch.float32 if op in _PROBE_F32 else (torch.int32 if op == "mbcnt" else torch.float64)
    a = np.ascontiguousarray(np.asarray(a, dtype=in_dt))

    def up(x, dt):
        if x is None:
            return None
        x = np.ascontiguousarray(np.asarray(x, dtype=dt))
        assert x.shape == a.shape
        return torch.from_numpy(x.view(np.int64) if dt == np.uint64 else x).to(dev)

    ta, tb, tc = up(a, in_dt), up(b, np.int32 if op == "mbcnt" else np.float64), up(c, np.float64)
    out = torch.empty(a.shape, dtype=out_dt, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = L.ionode_probe(PROBE_OPS[op], ptr(ta), ptr(tb), ptr(tc), out.data_ptr(), a.size, torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise ion.capi.IonodeError(f"ionode_probe({op}) failed ({rc})")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def probe_div_constf_sweep(ion, dev):
    """All 2^32 fp32 patterns through div_constf(x, 1000.0f, 0.001f) against the device's x / 1000.0f: (mismatches, patterns visited,
    bit-equal results)."""
    counts = torch.zeros(3, dtype=torch.int64, device=dev)
    rc = probe_lib(ion).ionode_probe_div_constf_sweep(counts.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise ion.capi.IonodeError(f"ionode_probe_div_constf_sweep failed ({rc})")
    torch.cuda.synchronize()
    return tuple(int(x) for x in counts.cpu())
