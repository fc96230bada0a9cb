"""Host tests (no GPU) of the split sampling run's cut: adf_split_choose_cut is host arithmetic inside the library
(csrc/stepper.hip) and engine.split_cut calls it.  The view's pointer offsets are formed inside adf_sample_split, next to
the device calls: tests/test_gpu_sample_split.py covers them."""
import ctypes as C

import pytest

from adsorbdiff_amd import lib as L
from adsorbdiff_amd.engine import split_cut


def _by_hand(natoms, edges=None):
    """The rule as the header states it, written the slow way."""
    if len(natoms) < 2:
        return 0
    best = None
    for c in range(1, len(natoms)):
        d = abs(sum(natoms[:c]) - sum(natoms[c:]))
        de = abs(sum(edges[:c]) - sum(edges[c:])) if edges is not None else 0
        if best is None or (d, de) < best[:2]:
            best = (d, de, c)
    return best[2]


@pytest.mark.parametrize("natoms, cut", [
    ([], 0), ([40], 0),                                   # fewer than two systems: no split
    ([31, 33], 1), ([31, 65, 290], 2), ([33, 64, 65, 97, 31], 3),
    ([10, 10, 10, 10], 2), ([10, 10, 10], 1),             # all equal: the middle; ties to the lowest boundary
    ([1000, 3, 4, 5], 1), ([3, 4, 5, 1000], 3), ([3, 1000, 4], 2),   # one giant system: alone, or with the lighter side
])
def test_cut_is_where_the_atom_counts_are_closest(natoms, cut):
    assert split_cut(natoms) == cut == _by_hand(natoms)
    if cut:
        assert 1 <= cut <= len(natoms) - 1


def test_edge_counts_break_ties_only():
    natoms = [10, 10, 10]                                 # boundaries 1 and 2 both differ by 10 atoms
    assert split_cut(natoms) == 1
    assert split_cut(natoms, [100, 1, 1]) == 1 and split_cut(natoms, [1, 1, 100]) == 2
    assert split_cut([10, 30, 10, 10], [1, 1, 1, 1000]) == 2 == _by_hand([10, 30, 10, 10])   # atoms decide first
    for n, e in (([7, 7, 7, 7, 7], [5, 9, 2, 8, 1]), ([4, 9, 4, 9], [3, 3, 3, 3])):
        assert split_cut(n, e) == _by_hand(n, e)
    with pytest.raises(ValueError):
        split_cut([1, 2], [1])
    with pytest.raises(ValueError):
        split_cut([1, -2])


def test_c_abi_of_the_five_split_entries():
    # the section "Two half-batches, two streams" of include/adsorbdiff_hip.h declares these five, in this order
    names = ["adf_painn_create_twin", "adf_painn_set_split", "adf_split_choose_cut", "adf_sample_split", "adf_split_stats"]
    first = L.EXPORTS.index(names[0])
    assert list(L.EXPORTS[first:first + len(names)]) == names
    i32, vp, batch = C.c_int32, C.c_void_p, C.POINTER(L.BatchDesc)
    assert L.SIGNATURES["adf_painn_create_twin"] == (i32, [vp, vp])
    assert L.SIGNATURES["adf_painn_set_split"] == (i32, [vp, i32])
    assert L.SIGNATURES["adf_split_choose_cut"] == (i32, [vp, vp, i32, vp])
    # the batch goes by reference; the view is a plain address (the engine hands over the address of its own SplitView)
    assert L.SIGNATURES["adf_sample_split"] == (i32, [vp, vp, batch, vp, vp, vp, vp, vp, i32, vp, vp, i32, i32, vp, vp, i32,
                                                      vp, vp, vp])
    assert L.SIGNATURES["adf_split_stats"] == (i32, [vp, vp, vp])
    lib = L.load()
    for name in names:
        fn = getattr(lib, name)
        assert fn.restype is L.SIGNATURES[name][0] and list(fn.argtypes) == L.SIGNATURES[name][1], name
    # argument checks come before any device work
    assert lib.adf_painn_create_twin(None, None) == L.ADF_EINVAL and lib.adf_painn_set_split(None, 1) == L.ADF_EINVAL
    cut = C.c_int32(-1)
    natoms = (C.c_int32 * 3)(31, 65, 290)
    assert lib.adf_split_choose_cut(natoms, None, 3, C.byref(cut)) == L.ADF_OK and cut.value == 2
