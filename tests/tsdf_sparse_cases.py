"""Cases and numpy helpers shared by tests/test_tsdf_sparse_cpu.py and tests/test_gpu_mesh_sparse.py: which bricks a set of grid points
with a negative update NEEDS (the bricks that meet its 3 x 3 x 3 dilation), allocation as ``SparseTsdfVolume.allocate`` does it, and
the fronto-parallel planes at brick boundaries that hold the mark to its tightness."""
import numpy as np

import tsdf_ref as R

BRICK_POINTS = 2048
SHAPES = {"16x16x8": (4, 4, 3), "64x4x8": (6, 2, 3)}               # log2 of the brick's points per axis
UPDATE_GRIDS = ((37, 21, 13), (40, 21, 13), (68, 9, 10))
THREE_POSES = ("identity", "tilted", "oblique")


def bricks_per_axis(dims, lg):
    return tuple(-(-d // (1 << l)) for d, l in zip(dims, lg))


def dilate(mask):
    """[nz, ny, nx] bool: the 3 x 3 x 3 index neighbourhood of ``mask``, clipped to the grid."""
    out = np.zeros_like(mask)
    nz, ny, nx = mask.shape
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                src = mask[max(0, -dz):nz - max(0, dz), max(0, -dy):ny - max(0, dy), max(0, -dx):nx - max(0, dx)]
                out[max(0, dz):nz - max(0, -dz), max(0, dy):ny - max(0, -dy), max(0, dx):nx - max(0, -dx)] |= src
    return out


def bricks_meeting(mask, lg):
    """Flat bool [bricks] (x fastest): the bricks that hold a point of ``mask`` ([nz, ny, nx])."""
    nz, ny, nx = mask.shape
    bx, by, bz = bricks_per_axis((nx, ny, nz), lg)
    padded = np.zeros((bz << lg[2], by << lg[1], bx << lg[0]), dtype=bool)
    padded[:nz, :ny, :nx] = mask
    return padded.reshape(bz, 1 << lg[2], by, 1 << lg[1], bx, 1 << lg[0]).any(axis=(1, 3, 5)).reshape(-1)


def needed_bricks(negative, lg):
    return bricks_meeting(dilate(negative), lg)


def point_offsets(dims, lg, directory):
    """int64 [nz, ny, nx]: the pool offset (slot 2048 + local) of every grid point, -1 where its brick has no slot."""
    nx, ny, nz = dims
    bx, by, _ = bricks_per_axis(dims, lg)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    brick = ((k >> lg[2]) * by + (j >> lg[1])) * bx + (i >> lg[0])
    local = (((k & ((1 << lg[2]) - 1)) << lg[1] | (j & ((1 << lg[1]) - 1))) << lg[0]) | (i & ((1 << lg[0]) - 1))
    slot = np.asarray(directory, dtype=np.int64)[brick]
    return np.where(slot >= 0, slot * BRICK_POINTS + local, -1)


def allocate(flags):
    """(directory int32 [bricks], brick_of_slot int32 [slots]) for the flagged bricks, in brick order."""
    new = np.asarray(flags) != 0
    directory = np.where(new, np.cumsum(new) - 1, -1).astype(np.int32)
    return directory, np.nonzero(new)[0].astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- planes at brick edges
AXIS_VOXEL, AXIS_TRUNC, AXIS_SIZE, AXIS_INTR = 0.05, 0.2, (72, 40), (60.0, 58.0, 35.5, 19.25)
# camera axes (rows of w2c's rotation) for a view along +x, +y, +z of the world: right-handed
_AXIS_ROWS = {0: ((0, 1, 0), (0, 0, 1), (1, 0, 0)), 1: ((0, 0, 1), (1, 0, 0), (0, 1, 0)), 2: ((1, 0, 0), (0, 1, 0), (0, 0, 1))}


def axis_case(axis, lg, first_of_next):
    """A flat plane seen along world axis ``axis`` from 1 m before a grid of two bricks and eight points per axis, placed a quarter
    voxel before grid layer L along the axis, so that L is the first layer behind the surface: the LAST layer of the first brick, or
    (``first_of_next``) the first layer of the second.  The band d < z <= d + trunc then holds layers L .. L + 3.  Returns a dict:
    dims, origin, voxel, trunc, intr, w2c (float64 4 x 4), out6 (float32 [6, H, W]), L."""
    dims = tuple(2 * (1 << l) + 8 for l in lg)
    origin = np.array((-0.913, -0.507, 0.811))
    L = (1 << lg[axis]) - 1 + (1 if first_of_next else 0)
    centre = origin + AXIS_VOXEL * (np.array(dims) - 1) / 2.0
    centre[axis] = origin[axis] - 1.0
    rot = np.array(_AXIS_ROWS[axis], dtype=np.float64)
    w2c = np.eye(4)
    w2c[:3, :3] = rot
    w2c[:3, 3] = -rot @ centre
    d = 1.0 + AXIS_VOXEL * (L - 0.25)
    W, H = AXIS_SIZE
    out6 = np.zeros((6, H, W), dtype=np.float32)
    out6[:3] = 0.5
    out6[3], out6[4], out6[5] = d, 1.0, d * d
    return dict(dims=dims, origin=tuple(origin), voxel=AXIS_VOXEL, trunc=AXIS_TRUNC, intr=AXIS_INTR, w2c=w2c, out6=out6, L=L, axis=axis)


def assert_mark_is_tight(case, lg, flags):
    """Every marked brick's index range along the view axis meets [L - 2, L + 3 + 2] (L .. L + 3: the layers in the band), and the
    grid's last brick along the axis -- it starts beyond L + 5 -- is not marked."""
    axis, L = case["axis"], case["L"]
    per = bricks_per_axis(case["dims"], lg)
    marked = np.asarray(flags).reshape(per[2], per[1], per[0]) != 0
    along = np.nonzero(marked.any(axis=tuple(a for a in range(3) if a != 2 - axis)))[0]      # (array axes are z, y, x)
    assert len(along) > 0
    B = 1 << lg[axis]
    for b in along:
        assert b * B <= L + 5 and b * B + B - 1 >= L - 2, (case["axis"], L, b)
    assert (per[axis] - 1) * B > L + 5 and per[axis] - 1 not in along


AXIS_CASES = [(axis, first_of_next) for axis in range(3) for first_of_next in (False, True)]
AXIS_IDS = [f"{'xyz'[a]}-{'first-of-next' if n else 'last-of-brick'}" for a, n in AXIS_CASES]
