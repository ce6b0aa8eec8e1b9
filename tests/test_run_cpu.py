"""The command line's handling of an experiment file (splatam_amd/run.py) without a GPU: loading the ``config`` dict from a Python
file, the defaults the reference fills in before its loop (scripts/splatam.py:458-464, 494-517, restated here), and the keys that stop
the run by name."""
import copy

import pytest

from splatam_amd import pipeline, run


def experiment(**data):
    cfg = pipeline.replica_config(tracking_iters=2, mapping_iters=2)
    cfg.update(workdir="w", run_name="r", use_wandb=False, load_checkpoint=False, eval_every=5, primary_device="cpu",
               data=dict(dict(basedir="b", sequence="s", desired_image_height=680, desired_image_width=1200, start=0, end=-1, stride=1,
                              num_frames=-1, dataset_name="replica"), **data))
    return cfg


def test_load_experiment_reads_the_config_dict(tmp_path):
    path = tmp_path / "splatam.py"
    path.write_text("seed = 7\nrun_name = f'room0_{seed}'\nconfig = dict(seed=seed, run_name=run_name, data=dict(num_frames=-1))\n")
    assert run.load_experiment(str(path)) == dict(seed=7, run_name="room0_7", data=dict(num_frames=-1))
    path.write_text("settings = {}\n")
    with pytest.raises(ValueError, match="config"):
        run.load_experiment(str(path))


def test_defaults():
    cfg = experiment()
    del cfg['tracking']['use_depth_loss_thres'], cfg['tracking']['depth_loss_thres'], cfg['gaussian_distribution']
    assert run.apply_defaults(cfg) == (False, False)
    assert cfg['tracking']['use_depth_loss_thres'] is False and cfg['tracking']['depth_loss_thres'] == 100000
    assert cfg['tracking']['visualize_tracking_loss'] is False and cfg['gaussian_distribution'] == "isotropic"
    data = cfg['data']
    assert data['ignore_bad'] is False and data['use_train_split'] is True
    assert (data['densification_image_height'], data['densification_image_width']) == (680, 1200)
    assert (data['tracking_image_height'], data['tracking_image_width']) == (680, 1200)
    # sizes of their own count only when they differ from the desired size
    assert run.apply_defaults(experiment(densification_image_height=340, densification_image_width=600,
                                         tracking_image_height=680, tracking_image_width=1200)) == (True, False)
    assert run.apply_defaults(experiment(tracking_image_height=340, tracking_image_width=600)) == (False, True)
    kept = experiment()
    kept['tracking'].update(use_depth_loss_thres=True, depth_loss_thres=20000)
    run.apply_defaults(kept)
    assert kept['tracking']['use_depth_loss_thres'] is True and kept['tracking']['depth_loss_thres'] == 20000


@pytest.mark.parametrize("change,key", (
    (lambda c: c.update(use_wandb=True), "use_wandb"),
    (lambda c: c.update(load_checkpoint=True), "load_checkpoint"),
    (lambda c: c['tracking'].update(visualize_tracking_loss=True), "visualize_tracking_loss"),
    (lambda c: c.update(mean_sq_dist_method="knn"), "mean_sq_dist_method"),
))
def test_keys_the_loop_cannot_honour_stop_the_run_by_name(change, key):
    cfg = experiment()
    run.apply_defaults(cfg)
    run.check_supported(copy.deepcopy(cfg))
    change(cfg)
    with pytest.raises(SystemExit, match=key):
        run.check_supported(cfg)
    with pytest.raises(SystemExit, match=key):
        run.run(cfg)                                        # ... before any file is touched
