"""The request generator of dp_requests_util.py, the oracle and the host build of the DP wrappers (emu_dp_batch in
tests/hostemu.cpp: staging buffers of str_cap characters, like the device's) proven against each other on the build box, before
test_gpu_dp_bodies.py sends the same requests to the device.  Bit-exact on all five result fields, no request left out."""
import ctypes as C

import numpy as np
import pytest

from circminer_amd import lib as cl
import dp_requests_util as dq


@pytest.fixture(scope="module")
def emu_dp(emu):
    emu.emu_dp_batch.restype = C.c_int
    emu.emu_dp_batch.argtypes = [C.POINTER(cl.Params), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_void_p]

    def run(b, fill, arrangement=0):
        out = np.zeros(len(b), cl.DP_RES_DTYPE)
        rc = emu.emu_dp_batch(C.byref(b.P), b.arena.ctypes.data, b.arena.size, b.req.ctypes.data, len(b), b.str_cap, fill, arrangement, out.ctypes.data)
        assert rc == 0, rc
        return out
    return run


@pytest.mark.parametrize("name", dq.ALL_BATCHES)
def test_emulation_equals_oracle(emu_dp, name):
    """every family through the wrappers' host build, under both buffer fills (on the host the fill is what a buffer holds beyond
    the staged codes, as on the device)"""
    b = dq.batch(name)
    assert len(b) > 0
    for fill in dq.FILLS:
        bad = b.first_mismatch(emu_dp(b, fill))
        assert bad is None, f"fill {fill:#010x}\n{bad}"


@pytest.mark.parametrize("name", dq.ARR1_BATCHES)
def test_emulation_resumable_form_equals_oracle(emu_dp, name):
    """kind 2 at band 3 through xdrop_w3_begin / _advance / _end, the form the heavy-pair pipeline's DP kernel runs"""
    b = dq.batch(name).kind2()
    assert len(b) > 0
    for fill in dq.FILLS:
        bad = b.first_mismatch(emu_dp(b, fill, 1))
        assert bad is None, f"fill {fill:#010x}\n{bad}"


def test_arena_layout():
    """every string has exactly 64 bytes on either side: the first at offset 64, the last ends 64 bytes before the arena does, and no
    view comes nearer than 64 bytes to its neighbours (the chunks are [pad][string][pad], back to back)"""
    b = dq.batch("b-3-144")
    q = b.req
    for off, step, ln in ((q["s_off"], q["s_step"], q["n"]), (q["t_off"], q["t_step"], q["m"])):
        lo = np.where(step > 0, off, off - ln + 1)
        assert lo.min() >= dq.PAD and (lo + ln).max() <= b.arena.size - dq.PAD
    first_lo = q["s_off"][0] if q["s_step"][0] > 0 else q["s_off"][0] - q["n"][0] + 1
    assert first_lo == dq.PAD
    last_lo = q["t_off"][-1] if q["t_step"][-1] > 0 else q["t_off"][-1] - q["m"][-1] + 1
    assert last_lo + q["m"][-1] == b.arena.size - dq.PAD


def test_hook_refuses_what_it_cannot_run(emu):
    """the checks cm_dp_batch makes before it launches (cmc::dp_req_check, shared with the emulation): CM_EINVAL"""
    b = dq.batch("d-3-8")
    emu.emu_dp_batch.restype = C.c_int
    emu.emu_dp_batch.argtypes = [C.POINTER(cl.Params), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_void_p]
    out = np.zeros(len(b), cl.DP_RES_DTYPE)

    def rc(P=b.P, arena_len=b.arena.size, req=b.req, cap=8, arr=0):
        return emu.emu_dp_batch(C.byref(P), b.arena.ctypes.data, arena_len, req.ctypes.data, len(req), cap, 0, arr, out.ctypes.data)

    assert rc() == 0
    for cap in (0, 4, 12, 1024):
        assert rc(cap=cap) == -1
    assert rc(arena_len=b.arena.size - 1) == -1            # the last view's pad leaves the arena
    bad = b.req.copy()
    bad["s_off"][0] = 63
    assert rc(req=bad) == -1
    bad = b.req.copy()
    bad["t_step"][0] = 2
    assert rc(req=bad) == -1
    bad = b.req.copy()
    bad["kind"][0] = 3
    assert rc(req=bad) == -1
    assert rc(arr=2) == -1
    assert rc(arr=1) == -1                                 # arrangement 1 takes kind 2 only
    assert rc(req=b.kind2().req, arr=1) == 0
    assert rc(P=dq.params(5, 8), req=b.kind2().req, arr=1) == -1      # ... and band 3 only


# ---- the generator is not vacuous: shares of family (a)'s requests by what the ORACLE answers (nothing here looks at the code under test)
def _shares(b):
    q, e, lrs = b.req, b.exp, b.lrs
    k2, k1 = q["kind"] == 2, q["kind"] == 1
    closed = np.array([r.kind == 2 and len(r.tv) >= 1 and len(r.sv) >= len(r.tv) and dq.same_prefix(r.sv, r.tv, len(r.tv)) for r in lrs])
    ok = e["ret"] <= b.P.max_ed
    n2, n1 = k2.sum(), k1.sum()
    return {"closed form taken": (closed & k2).sum() / n2,
            "ret > max_ed": (k2 & ~ok).sum() / n2,
            "success with indel != 0": (k2 & ok & (e["indel"] != 0)).sum() / n2,
            "success with sc_len > 0": (k2 & ok & (e["sc_len"] > 0)).sum() / n2,
            "0 < ret <= max_ed": (k2 & ok & (e["ret"] > 0)).sum() / n2,
            "kind 1 failures": (k1 & ~ok).sum() / n1,
            "kind 1 success with indel != 0": (k1 & ok & (e["indel"] != 0)).sum() / n1}


@pytest.mark.parametrize("band,max_ed", dq.PARAM_SETS)
def test_family_a_is_not_vacuous(band, max_ed):
    """4096 pairs per parameter set; each category at least 5 % of its kind's requests (`ret > max_ed` has no floor at (5, 8),
    where eight edits are allowed).  Measured when the generator was written, band 3 / 2 / 5, in per cent:
        closed form taken                 18.5 / 17.1 / 16.9
        ret > max_ed                      10.7 / 10.1 /  1.5
        success with indel != 0           28.3 / 34.6 / 18.5
        success with sc_len > 0           20.9 / 16.8 / 36.9
        0 < ret <= max_ed                 57.0 / 62.8 / 52.8
        kind 1 failures                   20.3 / 17.4 / 10.0
        kind 1 success with indel != 0    30.1 / 34.5 / 35.5
    If a floor fails, the generator is to be repaired, not the floor."""
    b = dq.batch(dq.A_BATCH[band])
    assert (b.req["kind"] == 2).sum() == 4096 and (b.exp["err"] == 0).all()
    sh = _shares(b)
    print(f"family (a) band {band} max_ed {max_ed}: " + ", ".join(f"{k} {100 * v:.1f} %" for k, v in sh.items()))
    for k, v in sh.items():
        if k == "ret > max_ed" and (band, max_ed) == (5, 8):
            continue
        assert v >= 0.05, (k, v)


def test_families_reach_their_edges():
    """what the smaller families are for is there: over-capacity requests with and without the error bit, strings of exactly
    str_cap characters, empty strings, every compare length of family (b)"""
    d = dq.batch("d-3-144")
    assert ((d.exp["err"] == dq.ERR_BAND).sum() >= 10) and ((d.exp["err"] == 0) & (np.maximum(d.req["n"], d.req["m"]) > 144)).sum() >= 10
    for cap in (144, 8, 1016):
        c = dq.batch(f"c-3-{cap}")
        assert (c.exp["err"] == 0).all()
        for kind in (0, 1, 2):
            k = c.req["kind"] == kind
            assert (np.maximum(c.req["n"], c.req["m"])[k] == cap).any(), (cap, kind)
        k2 = c.req["kind"] == 2
        assert ((c.req["n"] == cap) & (c.req["m"] == cap) & k2).any()
        assert (c.exp["ret"][k2] <= c.P.max_ed).any() and (cap == 8 or (c.exp["ret"][k2] > c.P.max_ed).any())     # (8 characters cannot fail)
    e = dq.batch("e-3-144")
    assert ((e.req["n"] == 0) & (e.req["m"] == 0)).any() and (e.req["n"] < e.req["m"]).any() and (e.req["s_mode"] == 2).any()
    bb = dq.batch("b-3-144")
    ham = (bb.req["kind"] == 0) & (bb.req["arg"] == 0)
    assert set(dq.B_LENGTHS) <= set(bb.req["n"][ham].tolist()) and {143, 144, 145, 300} <= set(bb.req["n"][ham].tolist())
    assert bb.exp["ret"][ham & (bb.req["n"] == 300)].max() >= 1
