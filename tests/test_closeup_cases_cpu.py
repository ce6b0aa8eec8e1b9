"""The walk-through scene of tests/closeup_cases.py, CPU only: what tests/test_gpu_closeup.py relies on is ASSERTED here for every
cell it uses --

  * every group of rows is populated (no comparison over a group passes on an empty set);
  * the scene's longest tile list lets the "auto" policy take its fast path;
  * the float32 oracle alone stays inside every bound the GPU test applies, with no outlier allowance used up;
  * the autograd oracle (oracle/raster_ref.py) and the C oracle (oracle/raster_ref.c), written independently, agree in this regime
    within the same bounds;
  * the group-wise gradient bound SEES the mistakes it is there for: three mutants of the C oracle (built from an edited copy of its
    source in a temporary directory) fail it by the factors recorded in profiles/closeup_scene.md."""
import os
import subprocess

import numpy as np
import pytest

from oracle import c_ref
from oracle import raster_ref as R
from tests import closeup_cases as cc
from tests.util import grad_scale

CELL_IDS = [f"{c[0]}-{'aniso' if c[5] else 'iso'}" for c in cc.CELLS]
GRAD_MAP = (('means3D', 'means3D'), ('means2D', 'means2D'), ('colors_precomp', 'colors'), ('opacities', 'opacities'),
            ('scales', 'scales'), ('rotations', 'rotations'))


@pytest.mark.parametrize("cell", cc.CELLS, ids=CELL_IDS)
def test_every_group_is_populated(cell):
    n, W = cell[0], cell[1]
    ref = cc.closeup_reference(*cell)
    g, radii = ref['groups'], ref['f64'][1]
    print({k: int(v.sum()) for k, v in g.items()}, "visible", int((radii > 0).sum()), "max radius", int(radii.max()))
    assert set(g) == set(cc.GROUPS)
    for k, least in cc.MIN_ROWS.items():
        assert int(g[k].sum()) >= least, (k, int(g[k].sum()))
    assert g['behind'].sum() >= 0.05 * n and g['plain'].sum() >= 20
    assert not (radii[g['behind']] > 0).any() and (radii[g['wide']] > W).all()
    # the masks are taken in float64: no live row sits so close to the guard band's edge or the 0.4 m line that float32 decides otherwise
    tv = cc.view_centres(ref['rv']['means3D'].numpy(), cc.walk_w2c())
    vis = tv[:, 2] > 0.2
    for axis, lim in ((0, R.FOV_GUARD * ref['cam'].tanfovx), (1, R.FOV_GUARD * ref['cam'].tanfovy)):
        assert np.abs(np.abs(tv[vis, axis] / tv[vis, 2]) / lim - 1.0).min() > 1e-5
    assert np.abs(tv[:, 2] / 0.2 - 1.0).min() > 1e-5
    # the clamped rows carry gradients of the frame's own magnitude: a wrong mask cannot hide under a tolerance from the tensor's maximum
    g64 = ref['f64'][3]
    for k in ('means3D', 'scales'):
        own = max(float(np.abs(g64[k][g[c]]).max()) for c in ('clamp_x', 'clamp_y', 'clamp_both'))
        assert own >= 0.3 * grad_scale(g64[k]), (k, own, grad_scale(g64[k]))


@pytest.mark.parametrize("cell", cc.CELLS, ids=CELL_IDS)
def test_scene_takes_the_fast_path(cell):
    from splatam_amd import rasterizer as rz
    cr = cc.closeup_reference(*cell)['f32'][4]
    longest = int(np.diff(cr.ranges()).max())
    print(f"num_rendered {cr.num_rendered()}, longest list {longest}")
    assert 0 < longest * rz.FAST_MARGIN <= rz.FAST_STRIDE, longest


def _assert_within_gpu_bounds(got_c, got_d, got_r, got_g, ref, what):
    """The bounds of tests/test_gpu_closeup.py with NO outlier allowance, against the float64 C oracle."""
    c64, r64, d64, g64, _ = ref['f64']
    assert np.array_equal(np.asarray(got_r), r64), what
    ec, ed = np.abs(np.asarray(got_c, dtype=np.float64) - c64).max(), np.abs(np.asarray(got_d, dtype=np.float64) - d64).max()
    print(f"{what}: colour max err {ec:.2e}, depth {ed:.2e}")
    assert ec <= 1e-4 and ed <= 1e-4, (what, ec, ed)
    for k in cc.GRAD_KEYS:
        if grad_scale(g64[k]) <= 1e-12 * grad_scale(g64['means3D']):          # (rotations of an isotropic map)
            assert float(np.abs(got_g[k]).max()) <= 1e-12 * grad_scale(g64['means3D']), k
            continue
        got = np.asarray(got_g[k], dtype=np.float64).reshape(g64[k].shape)
        e = float(np.abs(got - g64[k]).max()) / grad_scale(g64[k])
        print(f"{what}: grad {k} max err {e:.2e} of the tensor's max")
        assert e <= 1e-3, (what, k, e)
        cc.assert_groupwise(got, g64[k], ref['groups'], what=f"{what} grad {k}")
        assert float(np.abs(got[ref['groups']['behind']]).max()) == 0.0, k


@pytest.mark.parametrize("cell", cc.CELLS, ids=CELL_IDS)
def test_float32_oracle_alone_is_inside_every_bound(cell):
    ref = cc.closeup_reference(*cell)
    c32, r32, d32, g32, _ = ref['f32']
    _assert_within_gpu_bounds(c32, d32, r32, g32, ref, "float32 oracle vs float64 oracle")


@pytest.mark.parametrize("cell", cc.CELLS, ids=CELL_IDS)
def test_autograd_oracle_agrees_with_c_oracle(cell):
    ref = cc.closeup_reference(*cell)
    rv, cam, gout = ref['rv'], ref['cam'], ref['gout']
    inp = {k: v.clone().requires_grad_(True) for k, v in rv.items()}
    col, radii, dep, aux = R.rasterize(inp['means3D'], inp['means2D'], inp['opacities'], inp['colors_precomp'], inp['scales'],
                                       inp['rotations'], cam, return_aux=True)
    (col * gout).sum().backward()
    grads = {ok: inp[k].grad.numpy() for k, ok in GRAD_MAP}
    _assert_within_gpu_bounds(col.detach().numpy(), dep.numpy(), radii.numpy(), grads, ref, "autograd oracle vs float64 C oracle")
    cr = ref['f32'][4]
    assert np.array_equal(aux.tile_counts.numpy(), np.diff(cr.ranges()))
    assert (aux.n_contrib.numpy() != cr.n_contrib()).sum() <= 3


# -------------------------------------------------------------------------------------------------------------------------------
# sensitivity: the group-wise bound against three wrong oracles
# -------------------------------------------------------------------------------------------------------------------------------

MUTANTS = {
    # the adjoint's masks dropped: dL/dtx, dL/dty flow through a clamped centre
    "no gradient masks": [("real xmul = (txtz < -limx || txtz > limx) ? 0.f : 1.f, ymul = (tytz < -limy || tytz > limy) ? 0.f : 1.f;",
                           "real xmul = 1.f, ymul = 1.f;")],
    # the forward's Jacobian taken at the unclamped centre
    "no forward clamp": [("real tx = R_MIN(limx, R_MAX(-limx, txtz)) * tv[2];\n        real ty = R_MIN(limy, R_MAX(-limy, tytz)) * tv[2];",
                          "real tx = txtz * tv[2];\n        real ty = tytz * tv[2]; (void)limx; (void)limy;")],
    "near plane at 0.25": [("if (tv[2] <= 0.2f) continue;", "if (tv[2] <= 0.25f) continue;")],
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_groupwise_bound_catches_a_wrong_oracle(mutant, tmp_path, monkeypatch):
    """float32 mutant against the real float64 oracle, isotropic cell: the group-wise bound must fail, in a group the mistake touches."""
    src = open(os.path.join(os.path.dirname(c_ref.__file__), "raster_ref.c")).read()
    for old, new in MUTANTS[mutant]:
        assert src.count(old) == 1, (mutant, old)
        src = src.replace(old, new)
    (tmp_path / "mutant.c").write_text(src)
    so = str(tmp_path / "libmutant.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-fopenmp", "-ffp-contract=off", "-std=c11", "-shared", "-o", so, str(tmp_path / "mutant.c"), "-lm"])
    monkeypatch.setattr(c_ref, "_SO", so)
    monkeypatch.setattr(c_ref, "_libs", {})
    ref = cc.closeup_reference(*cc.CELLS[0])
    _, _, _, gm, _ = cc.oracle_run(ref['cam'], ref['rv'], ref['gout'], "f32")
    g64 = ref['f64'][3]
    worst = {}
    for k in ('means3D', 'means2D', 'colors', 'opacities', 'scales'):
        for grp, (factor, _) in cc.groupwise_excess(gm[k], g64[k], ref['groups']).items():
            worst[grp] = max(worst.get(grp, 0.0), factor)
        print(f"{mutant}: grad {k}: error / (1e-3 x the group's max) " + ", ".join(f"{g} {v[0]:.3g}" for g, v in cc.groupwise_excess(gm[k], g64[k], ref['groups']).items())
              + f"; of the tensor's max {np.abs(gm[k] - g64[k]).max() / (1e-3 * grad_scale(g64[k])):.3g}")
    print(f"{mutant}: worst factor per group {({g: round(v, 1) for g, v in worst.items()})}")
    hit = ('near',) if mutant == "near plane at 0.25" else ('clamp_x', 'clamp_y', 'clamp_both')
    for grp in hit:
        assert worst[grp] > 10.0, (mutant, grp, worst)
    if mutant == "no gradient masks":           # (the other two change the image, hence T for the rows behind: plain rows move too)
        assert worst['plain'] <= 1.0, (mutant, worst)
