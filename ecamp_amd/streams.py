"""The second streams of a step, in one place: who launches on which stream, what is held until when, who joins.

A step runs on three HIP streams: the main (compute) stream, the WEIGHT-GRADIENT stream (hip_ops.wgrad_group_async /
linear_wgrad_async, through `on_wgrad_stream`) and the BRANCH stream (the image decoder beside the report side, forward and
backward: `fork_branch` / `join_branch`, ECAMP.forward).  The main stream re-joins both at the end of a backward pass (`join`, an
autograd engine callback queued through `at_backward_end`); the data-parallel reducer makes its communication stream wait for
`others(device)` before a bucket's collective.  Tensors the weight-gradient stream reads are HELD (`held`) until events behind
the step have completed.  Pure torch: no ctypes, no kernel launch of its own."""
import collections

import torch

_second = {}   # ("wgrad" | "branch", device index) -> stream, created on first use (a process drives one device)


def _index(device):
    idx = torch.device(device).index
    return torch.cuda.current_device() if idx is None else idx


def second_stream(kind, device):
    key = (kind, _index(device))
    if key not in _second:
        _second[key] = torch.cuda.Stream(device=device)
    return _second[key]


def others(device):
    """Every stream other than the main one that may hold unfinished gradient work of `device`, of those created so far (weight-gradient
    stream, branch stream)."""
    return [_second[key] for key in (("wgrad", _index(device)), ("branch", _index(device))) if key in _second]


# --------------------------------------------------------------------------------------------- the end of a backward pass
_queued = {}   # fn -> id of the backward pass it is queued for


def at_backward_end(fn):
    """Queue `fn` on the autograd engine for the end of the backward pass this is called from, once per pass however often it is asked
    -> True; outside a backward pass nothing is queued -> False (the caller runs `fn`, or leaves it to someone who will).  What is
    remembered is WHICH pass `fn` was queued for, never a flag that only `fn` clears: the engine drops the callbacks of a pass that
    raised, and the next pass -- another id, failed passes included -- must queue again."""
    task = torch._C._current_graph_task_id()
    if task == -1:
        return False
    if _queued.get(fn) != task:
        for f in [f for f, t in _queued.items() if t != task]:   # earlier passes: over, whether or not their callbacks ran
            del _queued[f]
        torch.autograd.Variable._execution_engine.queue_callback(fn)
        _queued[fn] = task
    return True


def join():
    """The main stream waits for the second streams (end of backward; at once for a launch made outside a backward pass)."""
    cur = torch.cuda.current_stream()
    for st in others(torch.cuda.current_device()):
        cur.wait_stream(st)


# ---- tensors a second stream reads ------------------------------------------------------------------------------------------------
# `t.record_stream(side)` hands the question "when may this block be reused?" to the caching allocator: it answers with an event and keeps
# the block out of circulation until a LATER allocation call finds the event complete.  Which call that is depends on how far the host
# runs ahead of the GPU at that moment, so the allocator's steady state never quite arrives: round 6's bench record showed hipMalloc calls
# inside the timed steps in every run (7-107 even with the host's lead bounded), and one burst of them on a fresh box cost the host 87 ms
# and the GPU a step of 2x the median.  Instead the tensors are HELD here (a Python reference) until events recorded behind the step on
# every stream have completed, then dropped: the block goes back to the allocator the ordinary way, reusable at once by its own stream, and
# the step's allocation pattern is the same every step.  `seal()` is called where a step ends (FusedAdamW.pace) and by `hold` itself every
# 512 tensors or 8 GB (loops that never reach an optimizer); `reap()` drops what the GPU has finished.
def _record(st):
    ev = torch.cuda.Event()
    ev.record(st)
    return ev


class Held:
    """The tensors held for the second streams: one open set, and the sealed sets in seal order.  The three parameters are what it takes
    from torch -- `record(stream)` -> an event recorded there (`query`, `synchronize`), `current(device)` -> the current stream, `others` --
    and exist so that a test can hand it fakes."""

    def __init__(self, record=_record, current=torch.cuda.current_stream, others=others):
        self._record, self._current, self._others = record, current, others
        self._open, self._open_bytes = [], 0
        self._readers = []                  # the streams named as readers of the open set (hold's first argument)
        self._sealed = collections.deque()  # ([events], [tensors], bytes) in seal order
        self.bytes = 0                      # bytes of the sealed sets still held: behind steps the GPU has not finished
        #                                     (FusedAdamW.pace lets the host run fewer steps ahead when that is large)

    def hold(self, st, *tensors):
        """`st` (a second stream) reads `tensors`, which live in another stream's pool: keep them alive until that has happened.  Contract:
        every read of them by `st` has ALREADY been queued when this is called (the weight-gradient launches) -- a tensor that a second
        stream reads again later (the branch stream's backward nodes) must use record_stream, whose event is taken when the tensor is freed."""
        if all(st is not r for r in self._readers):
            self._readers.append(st)
        for t in tensors:
            if t is not None:
                self._open.append(t)
                self._open_bytes += t.numel() * t.element_size()
        if len(self._open) >= 512 or self._open_bytes > (8 << 30):   # loops that never reach an optimizer step (evaluation, tests): bounded all the same
            self.seal()
        elif self._sealed and (len(self._open) & 31) == 0:
            self.reap()

    def seal(self):
        """Close the open set behind an event on every stream that may read it -- the current one, every stream named as a reader since the
        last seal, and the second streams whatever was named, each once; drop the sets whose events have all completed."""
        if self._open:
            dev = self._readers[0].device
            streams = [self._current(dev)]
            for st in self._readers + self._others(dev):
                if all(st is not q and st != q for q in streams):
                    streams.append(st)
            self._sealed.append(([self._record(st) for st in streams], self._open, self._open_bytes))
            self.bytes += self._open_bytes
            self._open, self._open_bytes, self._readers = [], 0, []
        self.reap()

    def reap(self, block_first=False):
        """Drop the sealed sets the GPU is done with, oldest first; a finished set behind an unfinished one waits.  block_first: wait for
        the oldest one (tests)."""
        while self._sealed:
            evs, _, nb = self._sealed[0]
            if block_first:
                for e in evs:
                    e.synchronize()
                block_first = False
            if not all(e.query() for e in evs):
                break
            self._sealed.popleft()
            self.bytes -= nb


held = Held()   # the process-wide instance (optim._FlatOptimizer.pace seals and reaps it)


def on_wgrad_stream(device, launch, reads):
    """Run `launch()` on the weight-gradient stream of `device`, behind everything queued on the current stream so far; `reads` (one tuple
    per item of the launch: the tensors it reads) are held, and the main stream joins at the end of this backward pass -- at once when
    not inside one."""
    st = second_stream("wgrad", device)
    st.wait_stream(torch.cuda.current_stream())   # the operands (and earlier accumulations into the gradient) are ready
    with torch.cuda.stream(st):
        launch()
    for tensors in reads:
        held.hold(st, *tensors)   # the caching allocator must not recycle these while the weight-gradient stream reads them
    if not at_backward_end(join):
        join()


# --------------------------------------------------------------------------------------------- the image-decoder branch
def fork_branch(device, fn, reads):
    """-> fn() run on the branch stream of `device`, behind the main one."""
    bs = second_stream("branch", device)
    bs.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(bs):
        out = fn()
    for t in reads:
        t.record_stream(bs)   # (not held.hold: the branch's BACKWARD nodes read these again on `bs`, later than any fence taken here)
    return out


def join_branch(device, outs):
    """The main stream waits for the branch stream; `outs` are what the caller reads of the branch's results."""
    main = torch.cuda.current_stream(device)
    main.wait_stream(second_stream("branch", device))
    for t in outs:   # allocated on the branch stream and read by the CALLER on the main one, later than any point this function could
        t.record_stream(main)   # fence: the allocator's own bookkeeping (no effect on its steady state at this size: three scalars)
