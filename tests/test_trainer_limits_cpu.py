"""The oracle alone on the depth-8 / 96-feature data of tests/test_gpu_trainer_limits.py: its first tree must still
reach the paths that GPU test is there for, so a change to make_data or to the oracle cannot quietly take them away."""
import forest_train_oracle as oracle


def test_deep_wide_data_reaches_the_trainers_second_groups():
    x, y = oracle.deep_wide_data()
    (tree,), _ = oracle.train(x, y, 1, **oracle.DEEP)
    second_group, second_workgroup, deepest_leaves = oracle.deep_paths(tree)
    assert second_group > 0          # splits at heap ids 95..126: level 6's second histogram node group
    assert second_workgroup > 0      # splits at heap ids 191..254: level 7's second split workgroup
    assert deepest_leaves > 0        # leaves at level 8
    used = tree["feature"][tree["state"] == oracle.SPLIT]
    assert 0 in used and 95 not in used   # the copy of feature 0 loses every tie
