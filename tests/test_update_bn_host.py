"""model-update-bn (denet_amd/model/update_bn.py) without a GPU: the command line of the reference, the launcher and the rule
that picks the batch norms (denet/model/update_bn.py:20-27, :44-51)."""
import os

from denet_amd.model import update_bn, zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# denet/model/update_bn.py:20-27 - dest -> (default, required) - plus --seed of this project
REFERENCE_FLAGS = {
    "log_level": ("verbose", False),
    "model": (None, True),
    "output": (None, True),
    "input": (None, True),
    "extension": ("png", False),
    "batch_size": (128, False),
    "thread_num": (4, False),
}


def test_parser_matches_the_reference():
    parser = update_bn.build_parser()
    got = {a.dest: (a.default, a.required) for a in parser._actions if a.dest != "help"}
    assert got == dict(REFERENCE_FLAGS, seed=(None, False))
    args = parser.parse_args(["--model", "a", "--output", "b", "--input", "c", "--batch-size", "4", "--thread-num", "2",
                              "--seed", "7", "--extension", "npy"])
    assert (args.batch_size, args.thread_num, args.seed, args.extension) == (4, 2, 7, "npy")


def test_launcher_exists_and_is_executable():
    path = os.path.join(ROOT, "bin", "model-update-bn")
    assert os.path.isfile(path) and os.access(path, os.X_OK)
    assert "denet_amd.model.update_bn" in open(path).read()


def test_select_bn_layers_denet34_reference_order():
    """42 enabled batch norms: 7 top-level (stem BNA, two skip BNAs, four head BNAs) and 35 in the 16 resnet blocks (two per
    block plus the three projection shortcuts), in model order with each block's listed in its `layers` order"""
    model = zoo.denet34(2, "skip", 128)
    got = update_bn.select_bn_layers(model)
    expect = []
    for layer in model.layers:
        if layer.type_name in ("batchnorm", "batchnorm-relu"):
            expect.append(layer)
        elif layer.type_name == "resnet":
            expect += [l for l in layer.layers if l.type_name in ("batchnorm", "batchnorm-relu")]
    assert len(got) == 42 and all(a is b for a, b in zip(got, expect))
    assert sum(1 for l in got if any(l is t for t in model.layers)) == 7
    assert all(l.enabled for l in got)
    resnets = [l for l in model.layers if l.type_name == "resnet"]
    assert len(resnets) == 16 and sum(1 for r in resnets if len(r.layers) > r.n_main) == 3


def test_select_bn_layers_skips_disabled_and_other_nesting():
    """a disabled batch norm has no statistics; cifar3's three top-level `BN` layers are all taken"""
    model = zoo.cifar3(4)
    got = update_bn.select_bn_layers(model)
    assert [l.layer_index for l in got] == [l.layer_index for l in model.layers if l.type_name == "batchnorm"]
    assert len(got) == 3
    got[1].enabled = False
    chosen, skipped = update_bn._select(model)
    assert [l for l, _ in chosen] == [got[0], got[2]] and skipped == [got[1]]
