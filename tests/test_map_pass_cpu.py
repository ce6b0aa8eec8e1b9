"""``splatam_amd.map_pass`` (the list retry and the enqueue / read / redo driver every pass over a finished map goes through) and the
helpers of the ``params.npz`` reader (``splatam_amd.view``), on the host: fakes and CPU tensors, no device, no library."""
import numpy as np
import pytest
import torch

from splatam_amd import map_pass, view


# ---------------------------------------------------------------------------------------------------------------- fit_lists
def _renders(flags):
    """(render, digest, log) of a fake camera whose digests answer ``flags`` in turn."""
    log, answers = [], iter(flags)

    def render():
        log.append("render")

    def digest():
        log.append("digest")
        return next(answers)
    return render, digest, log


def test_fit_lists_stops_at_the_first_digest_that_fits():
    render, digest, log = _renders([False, True, True])
    assert map_pass.fit_lists(render, digest, "unused") is None
    assert log == ["render", "digest"]


def test_fit_lists_renders_three_times_and_raises_the_callers_message():
    render, digest, log = _renders([True] * 5)
    with pytest.raises(RuntimeError, match=r"^frame 7: the per-tile lists could not be sized for its view$"):
        map_pass.fit_lists(render, digest, "frame 7: the per-tile lists could not be sized for its view")
    assert log == ["render", "digest"] * 3


def test_fit_lists_fits_at_the_third_try():
    render, digest, log = _renders([True, True, False])
    map_pass.fit_lists(render, digest, "unused")
    assert log == ["render", "digest"] * 3


def test_fit_lists_never_digests_when_the_digest_says_so():
    """``view.render_trajectory`` in ``centers`` mode: its digest is ``mode != "centers" and view.check_overflow()``."""
    for mode, want in (("centers", ["render"]), ("color", ["render", "digest"] * 2)):
        render, check_overflow, log = _renders([True, False])
        map_pass.fit_lists(render, lambda: mode != "centers" and check_overflow(), "unused")
        assert log == want, mode


# ---------------------------------------------------------------------------------------------------------------- run_pass
def _pass(items, flagged):
    """``run_pass`` over ``items`` with a CPU table of one flag per item, as ``mesh._views_pass`` keeps it; returns (result, log)."""
    table = torch.zeros(len(items), dtype=torch.int64)
    log = []

    def enqueue(n, item):
        log.append(("enqueue", n, item))
        table[n] = int(item in flagged)

    def read():
        log.append(("read",))
        return [n for n, flag in enumerate(table.tolist()) if flag]

    def redo(n, item):
        log.append(("redo", n, item))
    return map_pass.run_pass(items, enqueue, read, redo), log


def test_run_pass_enqueues_everything_reads_once_and_redoes_the_flagged_in_order():
    items = ["a", "b", "c", "d", "e"]
    repeated, log = _pass(items, flagged={"d", "b"})
    assert log[:5] == [("enqueue", n, item) for n, item in enumerate(items)]       # every item, in order, before the read
    assert log[5] == ("read",) and log.count(("read",)) == 1
    assert log[6:] == [("redo", 1, "b"), ("redo", 3, "d")]                         # item order, through the driver's callback
    assert repeated == ["b", "d"]


def test_run_pass_orders_the_redos_by_item_whatever_order_read_reports():
    log = []
    repeated = map_pass.run_pass(range(10, 14), lambda n, item: None, lambda: [3, 0], lambda n, item: log.append((n, item)))
    assert log == [(0, 10), (3, 13)] and repeated == [10, 13]


def test_run_pass_without_flags_redoes_nothing():
    repeated, log = _pass([4, 9], flagged=set())
    assert repeated == [] and log == [("enqueue", 0, 4), ("enqueue", 1, 9), ("read",)]


def test_run_pass_without_items_still_reads_once():
    repeated, log = _pass([], flagged=set())
    assert repeated == [] and log == [("read",)]


def test_run_pass_takes_the_flag_from_a_slot_of_float64_rows():
    """The evaluations' table: the flag is one slot of each float64 row, and ``read`` is the only place the table becomes host data."""
    FLAGGED, frames = 5, [0, 4, 9]
    table = torch.zeros(len(frames), 8, dtype=torch.float64)
    host, again = {}, []

    def enqueue(n, t):
        table[n, 0] = 20.0 + t
        table[n, FLAGGED] = float(t == 4)

    def read():
        host['rows'] = table.numpy().copy()
        return [n for n in range(len(frames)) if host['rows'][n, FLAGGED] != 0]

    def redo(n, t):
        again.append(t)
        host['rows'][n] = [24.5, 0, 0, 0, 0, 0, 0, 0]
    assert map_pass.run_pass(frames, enqueue, read, redo) == [4] and again == [4]
    assert host['rows'][:, 0].tolist() == [20.0, 24.5, 29.0] and not host['rows'][:, FLAGGED].any()


# ---------------------------------------------------------------------------------------------------------------- the reader's helpers
def test_the_run_file_check_names_every_missing_key(tmp_path):
    path = str(tmp_path / "params.npz")
    np.savez(path, cam_trans=np.zeros((1, 3, 2)), intrinsics=np.eye(3), org_width=640)
    with np.load(path) as z:
        with pytest.raises(SystemExit) as failed:
            view._check_run_file(z, path)
    assert str(failed.value) == f"{path}: not a params.npz of a run (missing cam_unnorm_rots, w2c, org_height)"
    np.savez(path, cam_unnorm_rots=np.zeros((1, 4, 2)), cam_trans=np.zeros((1, 3, 2)), intrinsics=np.eye(3), w2c=np.eye(4), org_width=640, org_height=480)
    with np.load(path) as z:
        view._check_run_file(z, path)                                             # complete: nothing raised
        with pytest.raises(SystemExit, match=r"\(missing means3D, log_scales\)$"):
            view._check_run_file(z, path, ("means3D", "w2c", "log_scales"))


def test_intrinsics_scale_with_the_picture_size():
    """640 x 480 -> 320 x 120: fx and cx by 1/2, fy and cy by 1/4, as ``mesh._scaled_intrinsics`` gave them (exact powers of two)."""
    k = np.array([[600.0, 0.0, 319.5], [0.0, 604.0, 239.5], [0.0, 0.0, 1.0]])
    assert view._scaled_intrinsics(k, (320, 120), (640, 480)) == (300.0, 151.0, 159.75, 59.875)
    assert view._scaled_intrinsics((600.0, 604.0, 319.5, 239.5), (320, 120), (640, 480)) == (300.0, 151.0, 159.75, 59.875)
    assert view._scaled_intrinsics(k, (640, 480), (640, 480)) == (600.0, 604.0, 319.5, 239.5)
