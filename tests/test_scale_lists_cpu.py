"""Host-side invariants of the split-fp16 operand scale lists (include/ssv_hip.h, "Operand scales"): the LayerNorm / gate
backward kernels write ONE list entry and ONE partial row per tile of whichever kernel the shape picks, so for every shape the tile
count per item must fit the item's ssv_amax_rows(L) entries and the total must fit the `part` buffer, which callers size with
ssv_ln_partial_rows(B, L).  The library answers these queries without a device, so the whole dispatch table is swept here:
L = 1 .. 4200, the channel counts and batch sizes on both sides of every rule (16-column / wide / persistent kernels)."""
import pytest

from spoofsv_amd import _lib

CHANNELS = (64, 80, 128, 256, 512, 513)
BATCHES = (1, 2, 31, 32, 255, 256, 257)
LENGTHS = range(1, 4201)


def test_scale_list_length_is_four_entries_per_64_columns():
    L_ = _lib.lib()
    for L in LENGTHS:
        assert L_.ssv_amax_rows(L) == 4 * ((L + 63) // 64), L


@pytest.mark.parametrize("gate", [0, 1])
@pytest.mark.parametrize("C", CHANNELS)
def test_one_entry_and_one_partial_row_per_tile_fit_their_buffers(gate, C):
    """ssv_ln_bwd_partial_rows(gate, B, C, L, with_amax) is the tile count of the backward launch.  With a list: a multiple of B (the
    same tiles for every item) and per item <= ssv_amax_rows(L) -- a kernel writes entry `tile` of the item's list.  With and without:
    <= ssv_ln_partial_rows(B, L), the rows the caller's buffer has."""
    L_ = _lib.lib()
    rows, room, entries = L_.ssv_ln_bwd_partial_rows, L_.ssv_ln_partial_rows, L_.ssv_amax_rows
    for B in BATCHES:
        for L in LENGTHS:
            na, cap = entries(L), room(B, L)
            with_list, without = rows(gate, B, C, L, 1), rows(gate, B, C, L, 0)
            assert with_list > 0 and without > 0, (gate, B, C, L)
            assert with_list % B == 0 and with_list // B <= na, (gate, B, C, L, with_list, na)
            assert without % B == 0, (gate, B, C, L, without)
            assert with_list <= cap and without <= cap, (gate, B, C, L, with_list, without, cap)
