"""utils/graph.py::collector_off, the guard around every hipGraph capture: cyclic garbage (a dead trainer with its
captured graphs) is collected before the capture opens and the cycle collector stays off until it ends, so no
graph destructor can run inside another graph's capture."""
import gc
import weakref

import pytest

from pytorch_distributed_examples_amd.utils.graph import collector_off


class _Node:
    pass


def _dead_cycle():
    a, b = _Node(), _Node()
    a.other, b.other = b, a
    return weakref.ref(a)


def test_collects_on_entry_and_not_inside():
    assert gc.isenabled()
    before = _dead_cycle()
    with collector_off():
        assert before() is None
        assert not gc.isenabled()
        inside = _dead_cycle()
        junk = [[] for _ in range(20 * gc.get_threshold()[0])]  # enough container allocations for many young passes
        assert inside() is not None and len(junk) > 0
    assert gc.isenabled()
    gc.collect()
    assert inside() is None


def test_restores_the_collector_state():
    gc.disable()
    try:
        with collector_off():
            assert not gc.isenabled()
        assert not gc.isenabled()  # was off before: stays off
    finally:
        gc.enable()
    with pytest.raises(RuntimeError):
        with collector_off():
            raise RuntimeError("capture failed")
    assert gc.isenabled()
