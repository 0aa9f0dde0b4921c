"""The generated wrappers of cm_dispatch.cpp on a real context of each kernel build: arguments arrive in their places and the
call reaches the build the context was created for.  No kernel is launched."""
import ctypes as C

import numpy as np
import pytest

from circminer_amd import lib as cl

pytestmark = pytest.mark.gpu
CM_OK, CM_EINVAL, CM_ESTATE, CM_ELIMIT = 0, -1, -5, -6


@pytest.mark.parametrize("kmer,wide", [(20, False), (14, True)])      # 300 / 20 = 15 seeds: the 16-seed build; 300 / 14 = 21: the 24-seed build
def test_wrappers_reach_their_build(kmer, wide):
    hp = cl.HotPath(cl.default_params(kmer=kmer, max_read_len=300))
    try:
        L, h = hp.L, hp.h
        err = lambda: L.cm_last_error(h).decode()
        assert L.cm_load_contig(h, 99, C.byref(cl.IndexView())) == CM_EINVAL and "slot 99" in err(), err()
        assert L.cm_reads_swap(h) == CM_ESTATE and "no staged batch" in err(), err()
        assert L.cm_sync(h) == CM_OK and L.cm_reads_reset(h) == CM_OK and L.cm_prof_reset(h) == CM_OK
        ms, launches = (C.c_double * 8)(), (C.c_uint64 * 8)()
        assert L.cm_prof_get(h, ms, launches) == CM_OK
        ch, nc, hh = np.zeros(4 * cl.CM_BESTCHAINLIM, cl.CHAIN_DTYPE), np.zeros(4, np.int32), np.zeros(4, np.int32)
        rc = L.cm_chain_batch(h, 0, ch.ctypes.data, nc.ctypes.data, hh.ctypes.data)
        assert rc == (CM_ELIMIT if wide else CM_ESTATE)      # the narrow build is asked and has no contig in slot 0
        if not wide:
            assert "slot 0 not loaded" in err(), err()
    finally:
        hp.close()
