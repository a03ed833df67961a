"""The one storage model behind DeviceSlide / HostSlide (paths_amd/data_utils/slide.py: _Slide) and the one statement of the
storage-form rule (entry_name / index_args; csrc/select.hip: launch_gather / launch_level0), without a device."""
import itertools

import pytest
import torch

from paths_amd import _lib
from paths_amd.data_utils import slide as S

SHAPES, D = [(2, 3), (4, 6)], 8


def _slide(cls, packed: bool, masked: bool):
    """A slide of ``cls`` from CPU tensors through the private constructor: two levels, 2 x 3 and 4 x 6; the packed form keeps four
    rows of level 0 and none of level 1."""
    masks = [torch.ones(s, dtype=torch.uint8) for s in SHAPES]
    if packed:
        tables = dict(rows=[torch.ones(4, D), torch.zeros(0, D)],
                      index=[torch.tensor([[0, -1, 1], [2, 3, -1]], dtype=torch.int32), torch.full(SHAPES[1], -1, dtype=torch.int32)])
    else:
        tables = dict(grids=[torch.zeros(*s, D) for s in SHAPES])
    s = cls._new(torch.float32, torch.device("cpu"), masks, absmax=1.5, **tables)
    return s.with_masks([torch.zeros(sh, dtype=torch.uint8) for sh in SHAPES]) if masked else s


FORMS = list(itertools.product([S.DeviceSlide, S.HostSlide], [False, True], [False, True]))


@pytest.mark.parametrize("cls,packed,masked", FORMS)
def test_every_form_of_a_slide_has_the_same_attributes(cls, packed, masked):
    s = _slide(cls, packed, masked)
    assert type(s) is cls and set(vars(s)) == set(vars(_slide(S.DeviceSlide, False, False)))
    assert s.num_levels == 2 and [s.shape(l) for l in range(2)] == SHAPES and s.dim == D
    assert s.packed is packed and s.masked_view is masked and s.host_resident is (cls is S.HostSlide)
    assert s.synthetic_spec is None and s.dtype == torch.float32 and s.feature_absmax() == 1.5
    if packed:
        assert s.grids is None and len(s.rows) == len(s.index) == 2 and s.rows[1].shape == (0, D)
    else:
        assert s.rows is None and s.index is None and len(s.grids) == 2
    assert len(s.masks) == 2 and all(bool(m.any()) != masked for m in s.masks)


@pytest.mark.parametrize("name", ["paths_gather_rows", "paths_level0_batch"])
@pytest.mark.parametrize("packed,h16", list(itertools.product([False, True], repeat=2)))
def test_entry_names_are_entry_points_and_packed_forms_take_the_index(name, packed, h16):
    full = S.entry_name(name, h16, packed)
    assert full in _lib.SIGNATURES and full == name + ("_packed" if packed else "") + ("_h16" if h16 else "")
    table = torch.zeros(2, dtype=torch.int64) if packed else None
    assert len(S.index_args(table)) == (1 if packed else 0)
    assert len(_lib.SIGNATURES[full]) == len(_lib.SIGNATURES[name]) + len(S.index_args(table))
    batch = S._SlideBatch()
    batch.dtype, batch.packed, batch.index_ptrs = (torch.float16 if h16 else torch.float32), packed, [table]
    assert batch.entry(name) == full and len(batch.index_args(0)) == (1 if packed else 0)
    assert S.mask_kernel(batch.dtype) == "paths_tissue_mask_absmax" + ("_h16" if h16 else "") and S.mask_kernel(batch.dtype) in _lib.SIGNATURES


def test_the_eight_address_forming_entry_points_share_their_checks():
    """Host-side validation happens before any launch, so this is safe without a GPU: every call below is refused."""
    lib = _lib.load()
    A = 4096                                   # (an aligned non-null address: never dereferenced)

    def gather(full, packed, B, src_cell=A, index=A):
        # grid_ptrs, src_cell, D, state_cur, n_cur, ld_state_cur, src_row, Dp, num_out, B, n_next, fts_out, state_out, zero_pad, row_ptrs, zero_row
        args = [A, src_cell, 8, None, 4, 8, None, 8, A, B, 4, A, None, 0, None, None] + ([index] if packed else []) + [None]
        return getattr(lib, full)(*args)

    def level0(full, packed, B, gx=A, index=A):
        # grid_ptrs, gx, gy, B, D, patch_size, n0, fts, locs, parent, num_ims, zero_pad, row_ptrs, zero_row
        args = [A, gx, A, B, 8, 256, 6, A, A, A, A, 0, None, None] + ([index] if packed else []) + [None]
        return getattr(lib, full)(*args)

    for (name, call), packed, h16 in itertools.product([("paths_gather_rows", gather), ("paths_level0_batch", level0)], [False, True], [False, True]):
        full = S.entry_name(name, h16, packed)
        who = full[len("paths_"):].encode() + b":"
        assert call(full, packed, 0) != 0 and lib.paths_last_error().startswith(who) and b"bad shape" in lib.paths_last_error(), full
        # the dense forms refuse a null table like the packed ones
        assert call(full, packed, 2, None) != 0 and lib.paths_last_error().startswith(who) and b"null" in lib.paths_last_error(), full
        if packed:
            assert call(full, packed, 2, index=None) != 0 and lib.paths_last_error().startswith(who) and b"null" in lib.paths_last_error(), full
