"""The torch helper the distance and navigation fields share (stretch_mujoco_amd/datamodels.py: offsets_of_cells behind
nearest_offset() and next_offset()), on CPU tensors against the numpy expression.  No GPU."""
import numpy as np
import pytest
import torch

from stretch_mujoco_amd.datamodels import StatusStretchDistanceField, StatusStretchNavigationField, offsets_of_cells


def _fields(index):
    return (StatusStretchDistanceField(time=None, dist2=None, nearest=index, origin=(0.0, 0.0), cell=1.0, frame="grid"),
            StatusStretchNavigationField(time=None, potential=None, next=index, goal=None, origin=(0.0, 0.0), cell=1.0, frame="grid", neutral=50))


@pytest.mark.parametrize("ny,nx", [(1, 1), (3, 5)])
def test_offsets_of_cells_equals_the_numpy_expression(ny, nx):
    n = np.random.default_rng(10 * ny + nx).integers(-1, ny * nx, (2, ny, nx)).astype(np.int32)
    n[0].ravel()[0], n[1].ravel()[-1] = -1, ny * nx - 1      # a "none" and the last cell are there whatever the draw
    iy, ix = np.mgrid[0:ny, 0:nx]
    index = torch.tensor(n)
    got = offsets_of_cells(index)
    assert got.dtype == torch.int32 and tuple(got.shape) == (2, ny, nx, 2) and np.array_equal(index.numpy(), n)
    assert np.array_equal(got.numpy(), np.where((n >= 0)[..., None], np.stack((n // nx - iy, n % nx - ix), -1), 0)) and (got.numpy()[n == -1] == 0).all()
    df, nf = _fields(index)
    assert torch.equal(df.nearest_offset(), got) and torch.equal(nf.next_offset(), got)


def test_both_still_need_their_tensor():
    df, nf = _fields(None)
    with pytest.raises(ValueError, match="nearest=True"):
        df.nearest_offset()
    with pytest.raises(ValueError, match="next=True"):
        nf.next_offset()
