"""The DD_PRE_XCD block map of k_scatter_pre (dd_xcd_block_map in csrc/dd_internal.h,
exported as dd_pre_xcd_block_map). CPU only: the map is a __host__ __device__ function."""

import numpy as np

from datafusion_distributed_amd import api

NXCD = 8


def block_map(nblocks):
    out = np.full(nblocks, -1, dtype=np.int64)
    api.lib().dd_pre_xcd_block_map(nblocks, out.ctypes.data)
    return out


def test_xcd_map_is_a_bijection_with_contiguous_runs():
    """For every grid size 1..4100 (multiples of 8 or not): hardware blocks map one-to-one
    onto [0, nblocks); the blocks that share an L2 (equal b mod 8), taken in launch order,
    receive consecutive logical blocks; and the runs of the 8 residues tile [0, nblocks)
    in residue order."""
    for nblocks in range(1, 4101):
        m = block_map(nblocks)
        assert np.array_equal(np.sort(m), np.arange(nblocks)), nblocks
        nxt = 0
        for x in range(min(NXCD, nblocks)):
            run = m[x::NXCD]
            assert run[0] == nxt, (nblocks, x)
            assert np.array_equal(run, run[0] + np.arange(len(run))), (nblocks, x)
            nxt = run[-1] + 1
        assert nxt == nblocks
