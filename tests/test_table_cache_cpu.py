"""optim/_device.py on the host: ``TableCache``'s lifetime policy with plain objects as tables, a
counting ``build`` and a patched ``capturing``; and ``capturing`` itself for a CPU device."""
import pytest
import torch

from ddp_practice_amd.optim import _device as D

CPU = torch.device("cpu")


class _Builder:
    """``build`` of a lookup: a fresh object per call, counted."""

    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return object()


@pytest.fixture
def capture(monkeypatch):
    """``capture(True)`` / ``capture(False)``: what the module's ``capturing`` answers from here on."""
    state = {"on": False}
    monkeypatch.setattr(D, "capturing", lambda dev: state["on"])

    def set_(on):
        state["on"] = on

    return set_


def _key(numel=5):
    return ((0x1000, numel), (0x2000, 7))


def test_hit_returns_the_same_object_and_builds_once(capture):
    c, b = D.TableCache(), _Builder()
    t = c.get(_key(), b, CPU)
    assert c.get(_key(), b, CPU) is t
    assert b.calls == 1


def test_a_key_that_differs_in_one_numel_misses(capture):
    c, b = D.TableCache(), _Builder()
    t = c.get(_key(5), b, CPU)
    u = c.get(_key(6), b, CPU)
    assert u is not t and b.calls == 2
    assert c.get(_key(5), b, CPU) is t and b.calls == 2


def test_the_ninth_key_drops_the_first(capture):
    c, b = D.TableCache(), _Builder()
    first = c.get(0, b, CPU)
    for k in range(1, 9):
        c.get(k, b, CPU)
    assert b.calls == 9 and len(c.tables) == 8
    assert 0 not in c.tables and list(c.tables) == list(range(1, 9))
    again = c.get(0, b, CPU)
    assert b.calls == 10 and again is not first
    assert 1 not in c.tables and len(c.tables) == 8  # oldest first, again


def test_a_lookup_under_capture_pins_exactly_once(capture):
    c, b = D.TableCache(), _Builder()
    eager = c.get("eager", b, CPU)
    assert c.pinned == []
    capture(True)
    assert c.get("eager", b, CPU) is eager  # a hit of an eager-built entry
    assert [x is eager for x in c.pinned] == [True]
    built = c.get("captured", b, CPU)  # a build
    assert len(c.pinned) == 2 and c.pinned[1] is built
    c.get("eager", b, CPU)
    c.get("captured", b, CPU)
    assert len(c.pinned) == 2 and b.calls == 2


def test_an_evicted_pinned_table_stays_pinned(capture):
    c, b = D.TableCache(), _Builder()
    capture(True)
    t = c.get("captured", b, CPU)
    capture(False)
    for k in range(8):
        c.get(k, b, CPU)
    assert "captured" not in c.tables
    assert len(c.pinned) == 1 and c.pinned[0] is t


def test_nothing_is_pinned_outside_capture(capture):
    c, b = D.TableCache(), _Builder()
    for k in range(12):
        c.get(k, b, CPU)
        c.get(k, b, CPU)
    assert c.pinned == []


def test_two_caches_may_share_one_pinned_list(capture):
    a = D.TableCache()
    b = D.TableCache(a.pinned)
    capture(True)
    ta, tb = a.get(0, object, CPU), b.get(0, object, CPU)
    assert b.pinned is a.pinned and [x is y for x, y in zip(a.pinned, (ta, tb))] == [True, True]
    assert a.tables is not b.tables


def test_capturing_is_false_for_a_cpu_device(monkeypatch):
    def touched():
        raise AssertionError("torch.cuda state touched for a CPU device")

    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", touched)
    assert D.capturing(CPU) is False
    D.need_eager(CPU, "who", "what")  # no capture: no refusal


def test_the_refusal_names_owner_what_and_verb(capture):
    capture(True)
    with pytest.raises(RuntimeError, match=r"^EMA\.update: its words must exist before graph capture "
                                           r"\(run one eager update first\)$"):
        D.need_eager(CPU, "EMA.update", "its words", "update")
    with pytest.raises(RuntimeError, match="run one eager step first"):
        D.need_eager(CPU, "SGD", "its state")
