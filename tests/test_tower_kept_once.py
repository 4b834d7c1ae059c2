"""csrc/tower.h, TowerGeom::cut: the eight regions of a sample (up to 32 rows) overlap in what they compute of conv1 and conv2,
and the helper waves store every kept pixel from ONE of them.  Host only: the rectangles come from paac_tower_kept_layout, which
reads the constants the kernel reads."""
import ctypes

import numpy as np
import pytest

REGIONS = 8
LAYERS = [("conv1", 20, 0), ("conv2", 9, 8)]          # name, image size, offset of the layer's eight words in a region's sixteen


@pytest.fixture(scope="module")
def layout():
    from paac_amd import _lib
    out = (ctypes.c_int64 * (1 + 16 * REGIONS))()
    assert _lib.load().paac_tower_kept_layout(REGIONS, out, len(out)) == 0
    v = [int(x) for x in out]
    assert v[0] == REGIONS
    return np.array(v[1:], dtype=np.int64).reshape(REGIONS, 16)


@pytest.mark.parametrize("name,size,at", LAYERS)
def test_every_kept_pixel_has_one_owner(layout, name, size, at):
    owners = np.zeros((size, size), dtype=np.int64)
    for r in layout:
        oy, ox, oh, ow = r[at + 4:at + 8]
        assert oh > 0 and ow > 0 and oy >= 0 and ox >= 0 and oy + oh <= size and ox + ow <= size
        owners[oy:oy + oh, ox:ox + ow] += 1
    assert np.array_equal(owners, np.ones_like(owners)), name


@pytest.mark.parametrize("name,size,at", LAYERS)
def test_owned_rectangles_lie_inside_the_computed_ones(layout, name, size, at):
    for r in layout:
        cy, cx, ch, cw, oy, ox, oh, ow = r[at:at + 8]
        assert 0 <= cy and cy + ch <= size and 0 <= cx and cx + cw <= size
        assert cy <= oy and oy + oh <= cy + ch and cx <= ox and ox + ow <= cx + cw, (name, list(r[at:at + 8]))


@pytest.mark.parametrize("name,size,at", LAYERS)
def test_owners_are_balanced(layout, name, size, at):
    """Along an axis cut into n regions nobody owns more than ceil(size / n), plus one row or column of slack where the image does
    not divide."""
    ny, nx = len({int(r[at + 4]) for r in layout}), len({int(r[at + 5]) for r in layout})
    assert ny * nx == REGIONS
    for r in layout:
        oh, ow = r[at + 6:at + 8]
        assert oh <= -(-size // ny) + (1 if size % ny else 0)
        assert ow <= -(-size // nx) + (1 if size % nx else 0)


def test_only_the_eight_region_tower_is_reported():
    from paac_amd import _lib
    out = (ctypes.c_int64 * (1 + 16 * REGIONS))()
    assert _lib.load().paac_tower_kept_layout(4, out, len(out)) != 0
    assert _lib.load().paac_tower_kept_layout(REGIONS, out, 16 * REGIONS) != 0
