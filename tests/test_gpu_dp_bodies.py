"""The three alignment DPs of cm_core.h ON THE DEVICE, request by request, against the oracle (bit-exact on all five result
fields): cm_dp_batch runs the requests of dp_requests_util.py -- the ones test_dp_requests_cpu.py proves against the oracle through
the host emulation -- through what only the device build contains: the 16-byte staging loads with their byte swap and on-the-fly
complement, nibble packing into word-interleaved LDS, the SWAR compares of the closed forms with their tail masks, the band-3
X-drop loop that runs while any lane of the wave does, and its resumable arrangement in the heavy-pair pipeline.

Every comparison runs under two LDS fills (0x00000000 reads as eight matching 'A' codes, 0x45454545 as the two "other" codes
alternating): a dependence on LDS nobody staged can agree with the oracle under one content by accident.  Nothing is loaded but
the context.  A failing request is a complete reproducer: its strings and views are printed."""
import pytest

from circminer_amd import lib as cl
import dp_requests_util as dq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hp():
    h = cl.HotPath(cl.default_params())
    yield h
    h.close()


def _check(hp, b, fill, arrangement=0, grid=0):
    got = hp.dp_batch(b.P, b.arena, b.req, b.str_cap, fill, arrangement, grid)
    bad = b.first_mismatch(got)
    assert bad is None, f"fill {fill:#010x} arrangement {arrangement} grid {grid}\n{bad}"


@pytest.mark.parametrize("fill", dq.FILLS, ids=lambda f: f"fill{f:08x}")
@pytest.mark.parametrize("name", dq.ALL_BATCHES)
def test_wrappers_equal_oracle(hp, name, fill):
    """arrangement 0: the call as k_pair and k_hp_tasks make it, 64 different requests in flight per wave, one request per lane"""
    _check(hp, dq.batch(name), fill)


@pytest.mark.parametrize("fill", dq.FILLS, ids=lambda f: f"fill{f:08x}")
@pytest.mark.parametrize("name", dq.ARR1_BATCHES)
def test_resumable_form_equals_oracle(hp, name, fill):
    """arrangement 1: the loop of k_hp_dp -- lanes at different anti-diagonals, refilled from a shared cursor when 16 are idle"""
    b = dq.batch(name).kind2()
    _check(hp, b, fill, arrangement=1)
    _check(hp, b, fill, arrangement=1, grid=2)             # few waves: every lane is refilled many times


@pytest.mark.parametrize("fill", dq.FILLS, ids=lambda f: f"fill{f:08x}")
@pytest.mark.parametrize("band", [3, 2, 5])
def test_one_workgroup_runs_every_request(hp, band, fill):
    """family (a) with a grid of one workgroup: every lane runs some 190 requests one after the other and meets the previous
    request's staged strings in its buffers (test_wrappers_equal_oracle: as many workgroups as requests / 64, one request per lane)"""
    _check(hp, dq.batch(dq.A_BATCH[band]), fill, grid=1)


def test_hook_refuses_a_view_outside_the_arena(hp):
    b = dq.batch("d-3-8")
    bad = b.req.copy()
    bad["s_off"][0] = 63
    with pytest.raises(RuntimeError, match="cm_dp_batch"):
        hp.dp_batch(b.P, b.arena, bad, 8)
    with pytest.raises(RuntimeError, match="cm_dp_batch"):
        hp.dp_batch(b.P, b.arena, b.req, 12)
    assert len(hp.dp_batch(b.P, b.arena, b.req[:0], 8)) == 0
    _check(hp, b, 0)                                       # the context is as good as before
