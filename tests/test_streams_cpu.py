"""ecamp_amd/streams.py and the weight-gradient block of functions.py on the CPU: the held tensors against fake events and streams, the
end-of-backward request under CPU autograd, the block against a fake arena with `functions.ops` replaced by a recorder."""
import sys
import types

import pytest
import torch

from ecamp_amd import functions, streams
from ecamp_amd.arena import ParamArena


# ---------------------------------------------------------------------------------------------------------------- held tensors
class FakeStream:
    device = torch.device("cpu")

    def __init__(self, name):
        self.name = name


class FakeEvent:
    def __init__(self, stream):
        self.stream, self.done, self.waited = stream, False, 0

    def query(self):
        return self.done

    def synchronize(self):
        self.waited += 1
        self.done = True


class Rig:
    """A Held over fakes: `events` lists every event in the order it was recorded."""

    def __init__(self, second=()):
        self.main, self.second, self.events = FakeStream("main"), list(second), []
        self.held = streams.Held(record=self.record, current=lambda device: self.main, others=lambda device: list(self.second))

    def record(self, st):
        self.events.append(FakeEvent(st))
        return self.events[-1]

    def fenced(self, lo=0):
        return [e.stream.name for e in self.events[lo:]]


def _t(n=4):
    return torch.empty(n, dtype=torch.float32, device="meta")


def test_a_set_is_kept_while_any_event_is_incomplete_and_the_byte_count_returns_to_zero():
    w = FakeStream("wgrad")
    rig = Rig([w])
    rig.held.hold(w, _t(4), None, _t(6))   # None is skipped
    assert rig.held.bytes == 0 and rig.events == []
    rig.held.seal()
    assert rig.fenced() == ["main", "wgrad"] and rig.held.bytes == 40
    rig.events[0].done = True
    rig.held.reap()
    assert rig.held.bytes == 40, "one of two events complete: kept"
    rig.events[1].done = True
    rig.held.reap()
    assert rig.held.bytes == 0 and not rig.held._sealed
    rig.held.seal()
    assert len(rig.events) == 2, "nothing open: no event"


def test_a_complete_set_behind_an_incomplete_one_is_kept():
    w = FakeStream("wgrad")
    rig = Rig([w])
    rig.held.hold(w, _t(1))
    rig.held.seal()
    rig.held.hold(w, _t(2))
    rig.held.seal()
    assert rig.held.bytes == 12 and len(rig.events) == 4
    for e in rig.events[2:]:
        e.done = True
    rig.held.reap()
    assert rig.held.bytes == 12 and len(rig.held._sealed) == 2
    for e in rig.events[:2]:
        e.done = True
    rig.held.reap()
    assert rig.held.bytes == 0


def test_512_holds_seal_the_set_and_so_do_more_than_8_gib():
    w = FakeStream("wgrad")
    rig = Rig([w])
    for i in range(511):
        rig.held.hold(w, _t(1))
    assert rig.events == []
    rig.held.hold(w, _t(1))
    assert rig.fenced() == ["main", "wgrad"] and rig.held.bytes == 512 * 4 and rig.held._open == []
    rig = Rig([w])
    rig.held.hold(w, torch.empty(8 << 28, dtype=torch.float32, device="meta"))   # exactly 8 GiB: not above
    assert rig.events == []
    rig.held.hold(w, _t(1))
    assert rig.fenced() == ["main", "wgrad"] and rig.held.bytes == (8 << 30) + 4


def test_reap_is_tried_every_32_holds_while_sealed_sets_exist():
    w = FakeStream("wgrad")
    rig = Rig([w])
    rig.held.hold(w, _t(1))
    rig.held.seal()
    for e in rig.events:
        e.done = True
    for i in range(15):
        rig.held.hold(w, _t(1), _t(1))
    assert rig.held.bytes == 4, "30 holds: not tried"
    rig.held.hold(w, _t(1), _t(1))
    assert rig.held.bytes == 0, "32 holds: tried, and the finished set is gone"


def test_each_stream_is_fenced_once_whatever_was_named():
    w, b, x = FakeStream("wgrad"), FakeStream("branch"), FakeStream("other")
    rig = Rig([w, b])
    rig.held.hold(w, _t())
    rig.held.hold(x, _t())
    rig.held.hold(w, _t())          # named twice
    rig.held.hold(rig.main, _t())   # the current stream named as a reader
    rig.held.seal()
    assert rig.fenced() == ["main", "wgrad", "other", "branch"]
    rig.held.hold(x, _t())          # the readers of the last set are forgotten; the current and second streams are fenced all the same
    rig.held.seal()
    assert rig.fenced(4) == ["main", "other", "wgrad", "branch"]


def test_reap_block_first_waits_for_the_oldest_set_only():
    w = FakeStream("wgrad")
    rig = Rig([w])
    rig.held.hold(w, _t(1))
    rig.held.seal()
    rig.held.hold(w, _t(2))
    rig.held.seal()
    rig.held.reap(block_first=True)
    assert [e.waited for e in rig.events] == [1, 1, 0, 0] and rig.held.bytes == 8


# ---------------------------------------------------------------------------------------------------------------- at_backward_end
class _Ask(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fn, fail, seen):
        ctx.a = (fn, fail, seen)
        return x * 1

    @staticmethod
    def backward(ctx, g):
        fn, fail, seen = ctx.a
        seen.extend(streams.at_backward_end(fn) for _ in range(3))
        if fail:
            raise RuntimeError("this pass fails behind its first request")
        return g, None, None, None


def _pass(fn, fail=False):
    seen = []
    x = torch.ones(2, requires_grad=True)
    y = _Ask.apply(_Ask.apply(x, fn, fail, seen), fn, False, seen)   # two nodes ask, three times each
    y.sum().backward()
    return seen


def test_at_backward_end_queues_once_per_pass_and_reports_not_in_a_pass():
    ran = []
    fn = lambda: ran.append(1)
    assert streams.at_backward_end(fn) is False and ran == []
    assert _pass(fn) == [True] * 6 and ran == [1]
    assert _pass(fn) == [True] * 6 and ran == [1, 1]
    assert streams.at_backward_end(fn) is False and ran == [1, 1]


def test_after_a_pass_that_raised_the_next_pass_queues_again():
    """Guards the join of the weight-gradient stream (and the reducer's finalize) against a backward pass that raises: the engine never
    runs the callbacks such a pass queued, so a "queued" flag that only the callback clears stays set for the rest of the process and
    no later pass joins.  What is remembered is the pass, so the next pass queues again and its callback runs exactly once."""
    ran = []
    fn = lambda: ran.append(1)
    with pytest.raises(RuntimeError, match="fails behind its first request"):
        _pass(fn, fail=True)
    assert ran == [], "the engine drops the callbacks of a pass that raised"
    assert _pass(fn) == [True] * 6 and ran == [1]


# ---------------------------------------------------------------------------------------------------------------- the block
class FakeArena:
    """The arena as the block and _wgrad see it; `ready` is ParamArena's own."""
    ready = ParamArena.ready

    def __init__(self, log):
        self.deferred, self.log = None, log
        self.index = {id(sys.intern(n)): n for n in "abcdef"}   # the "parameters" are these names, a parameter's slot is its name
        self.on_ready = lambda slots: log.append(("ready", slots))

    def gradw(self, w, shape):
        return "g" + w, True


@pytest.fixture
def rec(monkeypatch):
    """functions.ops replaced by a recorder: every group qualifies; -> (log, arena, wgrad(name, arena=..., alpha_dev=...))."""
    log = []
    ops = types.SimpleNamespace(wgrad_group_supported=lambda items: True,
                                wgrad_group_async=lambda items, workgroups=0: log.append(("group", [it[2] for it in items])),
                                linear_wgrad_async=lambda dy, x, gw, alpha_dev=None, gb=None, accumulate=True: log.append(("linear", gw, alpha_dev)))
    monkeypatch.setattr(functions, "ops", ops)
    arena = FakeArena(log)
    return log, arena, lambda name, arena=arena, alpha_dev=None: functions._wgrad(arena, "dy", "x", name, alpha_dev=alpha_dev)


def test_a_block_issues_at_the_fourth_item_and_the_rest_at_exit(rec):
    log, A, wgrad = rec
    with functions._wgrad_block(A):
        for n in "abc":
            wgrad(n)
        assert log == []
        wgrad("d")
        assert log == [("group", ["ga", "gb", "gc", "gd"])]
        wgrad("e")
        wgrad("f")
        assert len(log) == 1
    assert log[1:] == [("group", ["ge", "gf"])] and functions._BLOCK is None
    del log[:]
    with functions._wgrad_block(A):
        wgrad("a")
        wgrad("b")
        wgrad("c")
        assert log == []
    assert log == [("group", ["ga", "gb", "gc"])]
    del log[:]
    with functions._wgrad_block(A):
        wgrad("a")
    assert log == [("linear", "ga", None)], "one item is no group"


def test_ready_is_forwarded_once_in_order_after_the_last_issue(rec):
    log, A, wgrad = rec
    with functions._wgrad_block(A):
        wgrad("a")
        wgrad("b")
        A.ready("b", "a")
        wgrad("c")
        wgrad("d")
        wgrad("e")
        A.ready("e", "c")
        assert [k for k, *_ in log] == ["group"]
    assert log == [("group", ["ga", "gb", "gc", "gd"]), ("linear", "ge", None), ("ready", ["b", "a", "e", "c"])]
    A.ready("d")
    assert log[-1] == ("ready", ["d"]) and A.deferred is None


def test_alpha_dev_and_foreign_arena_items_go_straight_through(rec):
    log, A, wgrad = rec
    other = FakeArena(log)
    with functions._wgrad_block(A) as blk:
        wgrad("a", alpha_dev="s")
        wgrad("b", arena=other)
        assert log == [("linear", "ga", "s"), ("linear", "gb", None)] and blk.items == []
        other.ready("b")
        assert log[-1] == ("ready", ["b"]), "another arena reports at once"


def test_nothing_is_issued_or_reported_after_an_exception(rec):
    log, A, wgrad = rec
    with pytest.raises(ValueError):
        with functions._wgrad_block(A):
            wgrad("a")
            wgrad("b")
            A.ready("a")
            raise ValueError("backward failed")
    assert log == [] and functions._BLOCK is None and A.deferred is None
    A.ready("b")
    assert log == [("ready", ["b"])]


def test_nesting_restores_the_outer_block(rec):
    log, A, wgrad = rec
    with functions._wgrad_block(A) as outer:
        wgrad("a")
        A.ready("a")
        with functions._wgrad_block(A) as inner:
            assert functions._BLOCK is inner and inner.prev is outer
            wgrad("b")
            wgrad("c")
            A.ready("c")
        assert functions._BLOCK is outer and A.deferred is outer.ready
        assert log == [("group", ["gb", "gc"])], "the inner block's items are issued at its exit; its ready calls wait for the outer one"
        wgrad("d")
    assert log[1:] == [("group", ["ga", "gd"]), ("ready", ["a", "c"])] and A.deferred is None
