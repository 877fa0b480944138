"""Clip sets on the host side (no GPU): the motion-file spec -> clips / per-type sets, and the integer rule that maps a reset's clip
draw onto a set entry (the kernels' reset_robot<true>)."""
import numpy as np
import pytest
import yaml

from openroborl_amd import _abi, config
from openroborl_amd.env import clip_draw_index, motion_spec


def test_scalar_path_is_a_set_of_one():
    assert motion_spec("laikago_pace", ["laikago"]) == (["laikago_pace"], {"laikago": [0]})
    assert motion_spec(["laikago_pace"], ["laikago"]) == (["laikago_pace"], {"laikago": [0]})


def test_list_is_the_clip_set_in_order():
    files, sets = motion_spec(["laikago_pace", "laikago_trot", "laikago_spin"], ["laikago"])
    assert files == ["laikago_pace", "laikago_trot", "laikago_spin"] and sets == {"laikago": [0, 1, 2]}


def test_duplicates_are_kept():
    files, sets = motion_spec(("laikago_pace", "laikago_pace"), ["laikago"])
    assert files == ["laikago_pace", "laikago_pace"] and sets == {"laikago": [0, 1]}


def test_nested_mixed_batch():
    files, sets = motion_spec([["laikago_pace", "laikago_trot"], "minicheetah_trot"], ["laikago", "mini_cheetah"], mixed=True)
    assert files == ["laikago_pace", "laikago_trot", "minicheetah_trot"]
    assert sets == {"laikago": [0, 1], "mini_cheetah": [2]}
    files, sets = motion_spec(["laikago_pace", "minicheetah_trot"], ["laikago", "mini_cheetah"], mixed=True)   # the old form
    assert files == ["laikago_pace", "minicheetah_trot"] and sets == {"laikago": [0], "mini_cheetah": [1]}


def test_yaml_list(tmp_path):
    p = tmp_path / "training_param.yaml"
    p.write_text(yaml.safe_dump({"imitation_learning_laikago": {"robot": "laikago", "motion_file": [
        "OpenRoboRL/envs/quadruped_robot/task/motions/laikago_pace.txt", "OpenRoboRL/envs/quadruped_robot/task/motions/laikago_trot.txt"]}}))
    params = config.load_training_params("imitation_learning_laikago", str(p))
    files, sets = motion_spec(params["motion_file"], [params["robot"]])
    assert [f.split("/")[-1] for f in files] == ["laikago_pace.txt", "laikago_trot.txt"] and sets == {"laikago": [0, 1]}


def test_errors():
    with pytest.raises(ValueError):
        motion_spec(["laikago_pace"] * (_abi.MAX_CLIPS + 1), ["laikago"])
    motion_spec(["laikago_pace"] * _abi.MAX_CLIPS, ["laikago"])                  # 16 is fine
    with pytest.raises(ValueError):
        motion_spec([["laikago_pace"] * 9, ["minicheetah_trot"] * 8], ["laikago", "mini_cheetah"], mixed=True)   # 17 in total
    with pytest.raises(ValueError):
        motion_spec([], ["laikago"])
    with pytest.raises(ValueError):
        motion_spec([[], "minicheetah_trot"], ["laikago", "mini_cheetah"], mixed=True)
    with pytest.raises(ValueError):
        motion_spec(["laikago_pace"], ["laikago", "mini_cheetah"], mixed=True)        # wrong count for a mixed batch
    with pytest.raises(ValueError):
        motion_spec("laikago_pace", ["laikago", "mini_cheetah"], mixed=True)
    with pytest.raises(ValueError):
        motion_spec([["laikago_pace", ["laikago_trot"]]], ["laikago"], mixed=True)   # a set is flat


def test_draw_to_index_is_uniform():
    """Over all 2^24 values of m, every entry of an n-clip set is picked floor(2^24 / n) or ceil(2^24 / n) times, n = 1 .. 16."""
    m = np.arange(1 << 24, dtype=np.int64)
    for n in range(1, _abi.MAX_CLIPS + 1):
        k = clip_draw_index(m, n)
        assert k.min() == 0 and k.max() == n - 1
        counts = np.bincount(k, minlength=n)
        assert counts.sum() == 1 << 24 and counts.max() - counts.min() <= 1, (n, counts.min(), counts.max())
        assert np.all(np.diff(k) >= 0)                     # monotone in the draw: entry k covers [k / n, (k + 1) / n) of [0, 1)


def test_draw_index_matches_the_float_draw():
    """m is recovered exactly from the float draw the kernels park in LDS (u = m / 2^24 is exact in float32)."""
    m = np.arange(0, 1 << 24, 4099, dtype=np.int64)
    u = m.astype(np.float32) * np.float32(1.0 / 16777216.0)
    assert np.array_equal((u * np.float32(16777216.0)).astype(np.int64), m)
