"""``slam.edit_schedule``: the one statement of when a ``pruning_dict`` / ``densify_dict`` edits the map, resets the opacities, and with
which thresholds, against tables written out here.  (That ``prune_gaussians`` and ``densify`` still compute the recorded results through
it is tests/test_slam_mirror.py's and tests/test_loop_golden.py's business.)"""
from splatam_amd import slam

A = dict(start_after=0, prune_every=20, stop_after=60, reset_opacities_every=500, reset_opacities=False, remove_big_after=0,
         removal_opacity_threshold=0.005, final_removal_opacity_threshold=0.005)
B = dict(start_after=5, densify_every=10, stop_after=30, reset_opacities_every=15, reset_opacities=True, remove_big_after=20,
         removal_opacity_threshold=0.005, final_removal_opacity_threshold=0.05)


def test_the_replica_pruning_schedule():
    for it in range(81):
        s = slam.edit_schedule(it, A, 'prune_every')
        assert s.active is (it <= 60), it
        assert s.edits is (it in (0, 20, 40, 60)), it
        assert s.resets is False, it
        assert s.opacity_threshold == 0.005 and s.remove_big is True, it


def test_a_schedule_with_a_late_start_resets_and_two_thresholds():
    for it in range(41):
        s = slam.edit_schedule(it, B, 'densify_every')
        assert s.active is (it <= 30), it
        assert s.edits is (it in (10, 20, 30)), it
        assert s.resets is (it in (15, 30)), it
        assert s.opacity_threshold == (0.05 if it == 30 else 0.005), it
        assert s.remove_big is (it >= 20), it
        if it > 30:
            assert not (s.active or s.edits or s.resets), it


def test_the_period_key_is_the_callers_and_a_truthy_reset_flag_counts():
    d = dict(B, prune_every=7, reset_opacities=1)
    assert [it for it in range(41) if slam.edit_schedule(it, d, 'prune_every').edits] == [7, 14, 21, 28]
    assert [it for it in range(41) if slam.edit_schedule(it, d, 'prune_every').resets is True] == [15, 30]
