"""The getting-started recipe (examples/simple-cifar10.sh) on the host: `same` convolutions with even filters, the `R.C` head
over a spatial logit map, the .mdl.gz round trip and the model-train command line. No GPU needed."""
import numpy as np
import pytest

from denet_amd.layer.convolution import ConvLayer
from denet_amd.layer.regression import RegressionLayer
from denet_amd.model import model_cnn, train, train_multi, zoo

RECIPE_FLAGS = ["--seed", "0", "--distort-mode", "o4", "--solver", "sgd", "--border-mode", "same", "--augment-mirror",
                "--activation", "relu", "--epochs", "90", "--batch-size", "32", "--train", "train_dir", "--test", "test_dir",
                "--extension", "png", "--learn-rate", "0.1", "--learn-momentum", "0.9", "--learn-anneal", "0.5",
                "--learn-anneal-epochs", "15", "30", "45", "60", "75", "--learn-decay", "0.0005", "--model-desc"]


def _convs(m):
    return [l for l in m.layers if isinstance(l, ConvLayer)]


def test_recipe_builds_with_same_border():
    m = zoo.simple_cifar10(4, 10, seed=1)
    assert m.layers[1].output_shape == (4, 3, 38, 38)
    convs = _convs(m)
    assert [l.output_shape[2] for l in convs] == [38, 38, 38, 19, 19, 19, 9, 9, 9, 4]
    assert [l.output_shape[3] for l in convs] == [38, 38, 38, 19, 19, 19, 9, 9, 9, 4]
    assert [l.filter_shape[2] for l in convs] == [3, 2, 1, 3, 2, 1, 3, 2, 1, 6]
    # the even filters pad k // 2 and keep the input's size; the others are unchanged
    assert [l.pad for l in convs] == [1, 1, 0, 1, 1, 0, 1, 1, 0, 0]
    assert [l.ohw for l in convs] == [None, (38, 38), None, None, (19, 19), None, None, (9, 9), None, None]
    assert convs[-1].border_mode == "valid" and convs[-1].output_shape == (4, 10, 4, 4)
    r = m.layers[-1]
    assert isinstance(r, RegressionLayer)
    assert r.valid == [(0, 2, 2)] and r.views == [2 * 4 + 2]
    assert r.output_shape == (4, 10) and r.log_pr_shape == (4, 10, 1)


def test_even_filter_same_against_half():
    """k = 2: `half` pads 1 all round (H + 1 outputs, as before), `same` drops the last row and column (H outputs)"""
    for border, size in (("half", 11), ("same", 10)):
        np.random.seed(0)
        m = model_cnn.ModelCNN()
        m.batch_size, m.class_num = 2, 4
        m.build("C[32,2] C[32,4] C[32,3]", (3, 10, 10), "relu", border, ["he-backward"])
        convs = _convs(m)
        if border == "half":
            assert [l.output_shape[2:] for l in convs] == [(11, 11), (12, 12), (12, 12)]
            assert all(l.ohw is None for l in convs)
        else:
            assert [l.output_shape[2:] for l in convs] == [(10, 10), (10, 10), (10, 10)]
            assert [l.pad for l in convs] == [1, 2, 1]
        assert convs[0].output_shape[2] == size


def test_same_even_needs_stride_one():
    np.random.seed(0)
    m = model_cnn.ModelCNN()
    m.batch_size, m.class_num = 2, 4
    with pytest.raises(AssertionError):
        m.build("C[32,2,2]", (3, 10, 10), "relu", "same", ["he-backward"])


def test_mdl_round_trip_keeps_border_and_valid(tmp_path):
    m = zoo.simple_cifar10(4, 10, seed=3)
    m.class_labels = {"c%i" % i: i for i in range(10)}
    path = str(tmp_path / "simple.mdl.gz")
    model_cnn.save_to_file(m, path)
    m2 = model_cnn.load_from_file(path, 4)
    assert [type(l) for l in m2.layers] == [type(l) for l in m.layers]
    assert [l.output_shape for l in m2.layers] == [l.output_shape for l in m.layers]
    for a, b in zip(_convs(m), _convs(m2)):
        assert b.border_mode == a.border_mode == "same" or b.border_mode == a.border_mode == "valid"
        assert b.ohw == a.ohw and b.pad == a.pad
        np.testing.assert_array_equal(b.omega.get_value(), a.omega.get_value())
    assert m2.layers[-1].valid == [(0, 2, 2)] and m2.layers[-1].views == [10]


def test_views_from_json_and_every_pixel():
    m = zoo.simple_cifar10(2, 6, seed=1)
    below = m.layers[:-1]
    r = RegressionLayer(below, use_center=True, json_param={"valid": [[0, 0, 3], [0, 3, 1]]})
    assert r.valid == [(0, 0, 3), (0, 3, 1)] and r.views == [3, 13] and r.log_pr_shape == (2, 6, 2)
    r = RegressionLayer(below, use_center=False, valid=[])
    assert r.views == list(range(16))


def test_duplicate_or_outside_views_rejected():
    m = zoo.simple_cifar10(2, 6, seed=1)
    with pytest.raises(ValueError, match="duplicate"):
        RegressionLayer(m.layers[:-1], use_center=False, valid=[(0, 1, 1), (0, 2, 2), (0, 1, 1)])
    with pytest.raises(ValueError, match="outside"):
        RegressionLayer(m.layers[:-1], use_center=False, valid=[(0, 4, 0)])


def test_training_over_several_views_raises():
    m = zoo.simple_cifar10(2, 6, seed=1)
    m.layers[-1] = RegressionLayer(m.layers[:-1], use_center=False, valid=[(0, 1, 1), (0, 2, 2)])
    with pytest.raises(NotImplementedError, match="one view"):
        m.build_train_func("sgd", skip_build=True)
    # one explicit view trains
    m.layers[-1] = RegressionLayer(m.layers[:-1], use_center=False, valid=[(0, 1, 3)])
    m.build_train_func("sgd", skip_build=True)
    assert m.cost_layers == [m.layers[-1]]


def test_recipe_command_line_parses():
    args = train.build_parser().parse_args(RECIPE_FLAGS + zoo.SIMPLE_CIFAR10_DESC.split())
    assert args.distort_mode == ["o4"] and args.border_mode == "same" and args.augment_mirror
    assert args.model_desc == zoo.SIMPLE_CIFAR10_DESC.split()
    assert args.learn_anneal_epochs == [15, 30, 45, 60, 75] and args.solver == "sgd"
    assert args.test_mode == "default" and not args.skip_train
    args = train.build_parser().parse_args(["--skip-train", "--test-mode", "single", "--distort-mode", "a", "b"])
    assert args.skip_train and args.test_mode == "single" and args.distort_mode == ["a", "b"]
    args = train_multi.build_parser().parse_args(RECIPE_FLAGS + zoo.SIMPLE_CIFAR10_DESC.split())
    assert args.distort_mode == ["o4"] and args.border_mode == "same"
