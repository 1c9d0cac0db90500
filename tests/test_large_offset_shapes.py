"""CPU checks of the shape arithmetic behind tests/test_gpu_large_offsets.py: the large shapes stay in the upper half of the 32-bit byte-offset
range, on the intended side of every size guard and within the device-memory budget, and the translated-blob regions stay clear of the faces
they must not reach."""
import pytest

import _large_shapes as L

IT3 = IT2 = L.IT          # PT iterations of the blob runs


def test_every_high_half_array_is_above_2_gib():
    for ni in (L.HIGH3, L.BELOW2, L.ABOVE2):
        assert L.smallest_bytes(ni) > L.HIGH_HALF_MIN, ni
        for name, ext in L.families(ni).items():
            assert L.nbytes(ext) > L.HIGH_HALF_MIN, (ni, name)
            assert L.cross_plane(ext) is not None, (ni, name)
    # the cell-centred array (nx ny nz 8 B) and the residuals, one entry shorter along one axis, are the smallest families
    nx, ny, nz = L.HIGH3
    assert nx * ny * nz * 8 > L.smallest_bytes(L.HIGH3) == nx * (ny - 1) * nz * 8 > L.HIGH_HALF_MIN


def test_3d_shape_sits_below_its_guards():
    assert L.fits_u32(L.HIGH3)                  # fused pipeline and z-marching sweeps run
    assert L.vep3_accepts(L.HIGH3)              # 3D VEP accepts the block
    assert L.cells_fit_i32(L.HIGH3)
    assert L.largest_bytes(L.HIGH3) < 1 << 32
    nx, ny, nz = L.HIGH3
    # the large-grid tile choices: > 384 wide and >= 384 deep (512-wide sweep tiles, 64 x 8 fused tiles, KZ = 12), no extent a multiple of a tile width
    assert nx > 384 and nz >= 384
    assert all(n % 64 and n % 8 for n in (nx, ny)) and nx % 512 and nz % 12


def test_2d_shapes_sit_on_either_side_of_the_batch_guard():
    assert L.batch2d(L.BELOW2) and not L.batch2d(L.ABOVE2)
    # just below: the batch form addresses to within 2 % of 4 GiB
    assert L.largest_bytes(L.BELOW2) < 1 << 32 and L.largest_bytes(L.BELOW2) > 0.98 * (1 << 32)
    (a, b), (c, d) = L.BELOW2, L.ABOVE2
    assert (a + 2) * (b + 2) > 0.98 * (1 << 29) and (c + 2) * (d + 2) < 1.01 * (1 << 29)


@pytest.mark.parametrize("ni", [L.HIGH3, L.BELOW2, L.ABOVE2])
def test_budgets_fit(ni):
    b = L.stokes3_budget() if len(ni) == 3 else L.stokes2_budget(ni)
    assert b <= L.BUDGET_BYTES, (ni, b / 1e9)
    assert L.BUDGET_BYTES < L.vep3_budget() <= L.VEP3_BUDGET_BYTES
    assert L.vep3_budget() > 216.2e9                     # the recorded peak of the VEP parity test
    # the recorded peaks of profiles/large_offsets_gpu.txt stay below what the skip condition counts
    assert L.stokes3_budget() > 178.4e9 and L.budget(L.HIGH3, L.STOKES3_ARRAYS) > 131.0e9
    assert L.stokes2_budget(L.BELOW2) > 177.8e9 and L.budget(L.BELOW2, L.STOKES2_ARRAYS) > 152.9e9


def test_cross_planes():
    # 3D cells: 2^28 entries / (770 * 598) per plane -> plane 582; the velocity families cross a few planes earlier, the residuals one later
    assert L.cross_plane(L.families(L.HIGH3)["cells"]) == 582
    assert L.cross_planes(L.HIGH3) == (579, 583)
    assert L.interior_box_start(L.HIGH3)[-1] == 578
    for name, ext in L.families(L.HIGH3).items():
        k = L.cross_plane(ext)
        plane = ext[0] * ext[1] * 8
        assert k * plane <= L.OFF31 < (k + 1) * plane, name
    for ni in (L.HIGH3, L.BELOW2, L.ABOVE2):
        assert L.straddles(ni), ni


@pytest.mark.parametrize("ni,it", [(L.HIGH3, IT3), (L.BELOW2, IT2), (L.ABOVE2, IT2)])
def test_blob_regions_stay_clear(ni, it):
    for name, disjoint, clear_lo, clear_hi in L.regions_clear(ni, it):
        assert disjoint and clear_lo and clear_hi, (ni, name)
    small = L.SMALL3 if len(ni) == 3 else L.SMALL2
    for name, corner_ok, interior_ok in L.small_regions_clear(small, it):
        assert corner_ok and interior_ok, (small, name)
    # the interior box keeps the radius it needs from the high faces in every family: the translated small run sees no face either
    st = L.interior_box_start(ni)
    for ext in L.families(ni).values():
        assert all(s + L.BOX + L.radius(it) < e for s, e in zip(st, ext))
        assert all(s - L.radius(it) > 0 for s in st)
