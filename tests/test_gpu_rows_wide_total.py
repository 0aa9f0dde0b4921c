"""The 64-bit total of the row formatters' driver (k_rows_total) on the device, for every entry point.

The driver sums a file's lengths in 64 bits where its bound on the file reaches 2^32 bytes:
    strings_max + items * (F::ITEM_FIXED_MAX + F::ITEM_CHRS * chr_max) >= 2^32,
chr_max being the longest name of the call's chromosome table, whether a state refers to it or not.  Here the table ends in one
entry no state refers to, with a name of L = 2^22 bytes, and the batch has n = 600 pairs, all of them active:
    cm_format_pam            items = n      ITEM_CHRS = 2 (cm_pam_text.h)     600 * 2 * 2^22 = 1200 * 2^22
    cm_format_sam            items = 2 n    ITEM_CHRS = 1 (cm_sam_text.h)    1200 * 1 * 2^22 = 1200 * 2^22
    cm_format_remain(_sorted) items = n     ITEM_CHRS = 2 (cm_remain_text.h)  600 * 2 * 2^22 = 1200 * 2^22   per file
and 1200 * 2^22 > 1024 * 2^22 = 2^32 before the other terms are counted (any n >= 512 would do).  With that name cut to one byte
the bound is a few hundred KB and the total is the scan's last word.  Both calls must give the same bytes, and those are the host
writer's, as in the formats' own tests.

The entry points give no view of which path a call took: nothing here observes that k_rows_total ran.  The arithmetic above is what
puts these calls on it; whoever changes the bound in RowsRun::lengths (cm_hot.hip) has to redo it, or the four tests become copies
of the narrow path's."""
import numpy as np
import pytest

from circminer_amd import lib as cl
from pam_text_util import CHRS, HostRows, directed_states, pair_text
from remain_sorted_util import check_sorted
from remain_text_util import HostRemain, key_value, remain_pair_text, remain_states
from sam_text_util import HostSam, sam_pair_text, sam_states

pytestmark = pytest.mark.gpu
N, LONG = 600, 1 << 22
EXTRA = len(CHRS)                                                           # the index of the entry no state refers to
SHORT = CHRS + [("N", 3, 7, 10)]
WIDE = CHRS + [("N" * LONG, 3, 7, 10)]
assert N * 2 * LONG >= 1 << 32 and 2 * N * LONG >= 1 << 32


def _past_the_table(st):
    """the states of the formats' tests print "-" for chr_id == len(CHRS); here that id has a name, so they move one up"""
    st["chr_id"] = np.where(st["chr_id"] == EXTRA, EXTRA + 1, st["chr_id"])
    assert not (st["chr_id"] == EXTRA).any() and (st["chr_id"] == EXTRA + 1).any() and (st["chr_id"] == EXTRA - 1).any()
    return st


@pytest.fixture(scope="module")
def hp(built):
    hp = cl.HotPath(cl.default_params())
    yield hp
    hp.close()


def _staged(hp, t1, t2, st, **bits):
    assert hp.stage_text(t1, t2, N, **bits)[0].n_pairs == N
    hp.swap()
    hp.poke_states(st)


def test_pam(hp, tmp_path):
    st = _past_the_table(directed_states(N))
    t1, t2 = pair_text(np.random.default_rng(1), N, (N // 2, N // 2 + 90))
    _staged(hp, t1, t2, st, keep_names=True)
    wide, short = hp.format_pam(WIDE), hp.format_pam(SHORT)
    assert wide == short and wide[1][:2] == [N, len(wide[0])]
    h = HostRows(tmp_path, t1, t2, N, chrs=SHORT)
    assert wide[0] == h.rows(st)
    h.close()


def test_sam(hp, tmp_path):
    st = _past_the_table(sam_states(N))
    t1, t2, _ = sam_pair_text(np.random.default_rng(2), N, st, (N // 2, N // 2 + 40))
    _staged(hp, t1, t2, st, keep_names=True, keep_quals=True)
    wide, short = hp.format_sam(WIDE), hp.format_sam(SHORT)
    assert wide == short and wide[1][:2] == [2 * N, len(wide[0])]
    h = HostSam(tmp_path, t1, t2, N, chrs=SHORT)
    assert wide[0] == h.rows(st)
    h.close()


@pytest.fixture(scope="module")
def remain_batch(hp, tmp_path_factory):
    st = _past_the_table(remain_states(N))
    t1, t2 = remain_pair_text(np.random.default_rng(3), N, (N // 2, N // 2 + 40))
    h = HostRemain(tmp_path_factory.mktemp("wide_remain"), t1, t2, N, chrs=SHORT)
    yield t1, t2, st, h
    h.close()


def test_remain(hp, remain_batch):
    t1, t2, st, h = remain_batch
    _staged(hp, t1, t2, st, keep_names=True, keep_quals=True, keep_names2=True)
    wide, short = hp.format_remain(WIDE, keys=True), hp.format_remain(SHORT, keys=True)
    assert wide[:2] == short[:2] and np.array_equal(wide[2], short[2]) and wide[3:] == short[3:]
    assert wide[3] == N and wide[4][:2] == [2 * N, len(wide[0]) + len(wide[1])]
    assert wide[:2] == h.files(st, np.arange(N), chrs=SHORT)
    assert wide[2].tolist() == [key_value(st[i], SHORT) for i in range(N)]


def test_remain_sorted(hp, remain_batch, monkeypatch):
    monkeypatch.delenv("CM_REMAIN_TIE_CAP", raising=False)
    t1, t2, st, h = remain_batch
    _staged(hp, t1, t2, st, keep_names=True, keep_quals=True, keep_names2=True)
    wide, short = hp.format_remain_sorted(WIDE), hp.format_remain_sorted(SHORT)
    assert wide[:2] == short[:2] and np.array_equal(wide[2], short[2]) and all(np.array_equal(a, b) for a, b in zip(wide[3], short[3])) and wide[4:] == short[4:]
    assert wide[4] == N and wide[5][:2] == [2 * N, len(wide[0]) + len(wide[1])]
    check_sorted(wide[0], wide[1], wide[2], wide[3], h, st, np.arange(N), chrs=SHORT)
