"""ops.switches / ops.algorithms: the block form of "set a module global of ops, put it back" (host only, no device call).

The algorithm tables are emptied of the committed tuned file for the whole module (DENET_TUNE_CACHE=0 semantics through the module
globals), so that _load_tuned_once() never reaches the library."""
import pytest

from denet_amd import ops

G = (1, 8, 8, 32, 32, 3, 3, 3, 1, 1, 8, 8)          # a geometry; nothing is launched at it
G2 = (2, 8, 8, 32, 32, 3, 3, 3, 1, 1, 8, 8)


@pytest.fixture(autouse=True)
def _no_tuned_file(monkeypatch):
    monkeypatch.setattr(ops, "_TUNE_LOADED", True)
    monkeypatch.setattr(ops, "POLICY", None)
    wino, tuned = dict(ops._WINO), set(ops._TUNED)
    yield
    assert ops._WINO == wino and ops._TUNED == tuned      # every test of this file leaves the tables as it found them


def _snapshot():
    return {k: v for k, v in vars(ops).items() if not k.startswith("__")}


# ------------------------------------------------------------------------------------------------- switches
def test_switches_sets_and_restores():
    was = (ops.DGRAD_T, ops.BWD_SUMS)
    with ops.switches(DGRAD_T=not was[0], BWD_SUMS=was[1] + 1):
        assert (ops.DGRAD_T, ops.BWD_SUMS) == (not was[0], was[1] + 1)
    assert (ops.DGRAD_T, ops.BWD_SUMS) == was


def test_switches_restores_after_an_exception():
    was = ops.AUTOTUNE
    with pytest.raises(RuntimeError, match="inside"):
        with ops.switches(AUTOTUNE=not was):
            assert ops.AUTOTUNE == (not was)
            raise RuntimeError("inside")
    assert ops.AUTOTUNE == was


@pytest.mark.parametrize("name,error,match", [
    ("DGRAD_TT", AttributeError, "DGRAD_TT"),                  # a typo must not create a global
    ("static_policy", AttributeError, "static_policy"),        # a function
    ("switches", AttributeError, "switches"),
    ("LaunchTrace", AttributeError, "LaunchTrace"),            # a class
    ("os", AttributeError, "os"),                              # a module
    ("FINAL_FOLD", ValueError, "set_final_fold"),              # lives on the C side too: its setter is named
])
def test_switches_refuses_and_changes_nothing(name, error, match):
    before = _snapshot()
    entered = []
    with pytest.raises(error, match=match):
        with ops.switches(**{"DGRAD_T": not ops.DGRAD_T, name: 1}):          # the good name in front is not applied either
            entered.append(1)
    assert not entered
    after = _snapshot()
    assert after.keys() == before.keys() and all(after[k] is before[k] for k in before)


def test_switches_nest():
    was = ops.WINO4T
    with ops.switches(WINO4T=1):
        with ops.switches(WINO4T=2, DGRAD_S2=False):
            assert (ops.WINO4T, ops.DGRAD_S2) == (2, False)
        assert ops.WINO4T == 1
    assert ops.WINO4T == was


def test_switches_takes_a_policy_that_holds_a_function():
    with ops.switches(POLICY=ops.static_policy):
        with ops.switches(POLICY=None):                 # (POLICY holds a function now, and is still a switch)
            assert ops.POLICY is None
        assert ops.POLICY is ops.static_policy
    assert ops.POLICY is None


# ------------------------------------------------------------------------------------------------- algorithms
def test_algorithms_restores_after_an_exception():
    table, wino, tuned = ops._WINO, dict(ops._WINO), set(ops._TUNED)
    with pytest.raises(RuntimeError, match="inside"):
        with ops.algorithms(POLICY=ops.direct_policy):
            ops._WINO[(0, G)] = 4
            ops._TUNED.add((0, G))
            setattr(ops, "POLICY", ops.static_policy)   # set by hand in the block: put back all the same
            raise RuntimeError("inside")
    assert ops.POLICY is None and ops._WINO is table and ops._WINO == wino and ops._TUNED == tuned


def test_algorithms_table_replaces_and_restores():
    table = ops._WINO
    with ops.algorithms():
        ops._WINO[(0, G)] = 2
        with ops.algorithms(table={(1, G): 4}) as live:
            assert live is ops._WINO is table and dict(live) == {(1, G): 4}
            live[(2, G)] = 0                            # the yielded dict is the live table: _decided reads it
            assert ops._decided(2, G) == 0
            del live[(1, G)]
            assert (1, G) not in ops._WINO
        assert ops._WINO is table and ops._WINO[(0, G)] == 2 and (1, G) not in ops._WINO and (2, G) not in ops._WINO
        with ops.algorithms(table={}):
            assert ops._WINO == {}
        assert ops._WINO[(0, G)] == 2


def test_algorithms_drops_decisions_made_inside():
    with ops.algorithms(table={}, POLICY=ops.direct_policy):
        assert ops._decided(0, G) == 0 and ops._WINO[(0, G)] == 0          # made before the inner block
        with ops.algorithms(POLICY=lambda mode, g: 2, AUTOTUNE=True):
            assert ops.AUTOTUNE is True
            assert ops._decided(0, G2) == 2 and (0, G2) in ops._WINO
            assert ops._decided(0, G) == 0                                 # decided already: the policy is not asked again
        assert (0, G2) not in ops._WINO and ops._WINO[(0, G)] == 0
        assert ops.POLICY is ops.direct_policy
        assert ops._decided(0, G2) == 0                                    # decided afresh, by the outer block's policy
    assert (0, G) not in ops._WINO and (0, G2) not in ops._WINO


def test_algorithms_refuses_a_bad_switch_and_changes_nothing():
    wino = dict(ops._WINO)
    with pytest.raises(AttributeError, match="AUTOTUNED"):
        with ops.algorithms(table={(0, G): 4}, AUTOTUNED=False):
            raise AssertionError("entered")
    assert ops._WINO == wino and ops.POLICY is None


def test_direct_policy():
    assert [ops.direct_policy(mode, G) for mode in (0, 1, 2, 3)] == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------- the named blocks over them
def test_infer_fold_and_cluster_device_coerce_and_restore():
    for block, name in ((ops.infer_fold, "INFER_FOLD"), (ops.cluster_device, "CLUSTER_DEVICE")):
        was = getattr(ops, name)
        for value in (0, 1, "yes", None):
            with block(value):
                assert getattr(ops, name) is bool(value)
                with block(not value):
                    assert getattr(ops, name) is (not value)
                assert getattr(ops, name) is bool(value)
            assert getattr(ops, name) is was
        with pytest.raises(RuntimeError):
            with block(not was):
                raise RuntimeError("inside")
        assert getattr(ops, name) is was


def test_precision_blocks_set_restore_and_refuse():
    for block, name, what, flag in ((ops.infer_precision, "INFER_PRECISION", "inference", ops.infer_bf16),
                                    (ops.train_precision, "TRAIN_PRECISION", "training", ops.train_bf16)):
        was = getattr(ops, name)
        with block("bf16"):
            assert getattr(ops, name) == "bf16" and flag()
            with block("fp32"):
                assert getattr(ops, name) == "fp32" and not flag()
            assert getattr(ops, name) == "bf16"
        assert getattr(ops, name) == was
        with pytest.raises(ValueError, match=r"%s precision 'fp16': expected one of fp32, bf16" % what):
            with block("fp16"):
                raise AssertionError("entered")
        assert getattr(ops, name) == was
