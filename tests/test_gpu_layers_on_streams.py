"""The differentiable layers on a side stream and inside a captured graph (the table: tests/layers_on_streams_cases.py).

``_C.stream()`` hands torch's *current* stream to every entry point, and the multi-launch layers chain their launches through a workspace
on that stream.  Every other test launches on the default stream, eagerly: a single launch -- or memset, or copy -- that landed on stream 0
instead, a host read in the middle of a call, or a call that cannot be captured would pass them all.

No tolerance anywhere: every comparison is ``torch.equal`` against an eager run of the same code on the default stream (whose numbers the
sweeps hold to fp64).

Test 1, a side stream whose inputs arrive late.  The operands are allocated afresh and filled with NaN; on a side stream (the fixture
``side``: one that does not share the default stream's hardware queue) a delay (a chain of matmuls, tens of milliseconds), then the copies
of the real values, then the call are queued, and nothing on the default stream waits for that stream.  Whatever the call puts on stream
0 runs at once and reads NaN.  The test shows its own sensitivity: a clone of an operand buffer taken on the default stream when the call
is issued must still hold NaN, otherwise the case fails as inconclusive (the delay was over before the call was queued).  A second clone,
taken when the call has returned, must hold NaN too: if only that one holds the values, the call made the host wait for its stream -- a
device-to-host read or a synchronisation inside a layer.

Test 2, captured and replayed queued.  The call is captured under ``torch.cuda.graph`` as one linear chain (after an eager warm-up on the
capture stream); then, with no host synchronisation in between, six times: copy data set A or B into the static buffers, replay, clone the
outputs.  Each clone has the bits of the eager run on that data set.  A case that cannot be captured fails.  Six is a fixed count.  The
optimisers are not captured: they take the step number by value (hypad_amd/optim.py).
"""
import math

import pytest
import torch

import layers_on_streams_cases as lc

pytestmark = pytest.mark.gpu

NAN = float("nan")
DELAY_N, DELAY_MATMULS = 4096, 24
REPLAYS = 6

_CASES = {}


def _case(name):
    if not _CASES:
        _CASES.update({c.name: c for c in lc.cases()})
    return _CASES[name]


def _buffers(host):
    return list(host)                                       # (the keys of ops that start with "_" are objects, not buffers)


def _load(ops, src):
    with torch.no_grad():
        for k in src:
            ops[k].copy_(src[k])


def _eager(case, host):
    """The case on the default stream, from freshly placed buffers; returns clones, with everything finished."""
    ops = case.place(host)
    _load(ops, host)
    torch.cuda.synchronize()
    want = [t.detach().clone() for t in case.run(ops)]
    torch.cuda.synchronize()
    for i, t in enumerate(want):
        assert bool(torch.isfinite(t).all()), f"{case.name}: tensor {i} of the eager run is not finite (the data must stay clear of NaN)"
    return want


def _differing(got, want):
    return [f"tensor {i} {tuple(w.shape)}: {int((g != w).sum())} of {w.numel()} elements differ" + (" (NaN in it)" if bool(torch.isnan(g).any()) else "")
            for i, (g, w) in enumerate(zip(got, want)) if g.shape != w.shape or not torch.equal(g, w)]


@pytest.fixture(scope="module")
def delay():
    """queue() puts the delay on the current stream; .ms is its duration, measured once with events on an otherwise idle device."""
    a = torch.randn(DELAY_N, DELAY_N, device="cuda") / math.sqrt(DELAY_N)
    b, c = torch.randn(DELAY_N, DELAY_N, device="cuda") / math.sqrt(DELAY_N), torch.empty(DELAY_N, DELAY_N, device="cuda")

    def queue():
        for _ in range(DELAY_MATMULS // 2):
            torch.mm(a, b, out=c)
            torch.mm(c, b, out=a)
    queue()                                                 # (the BLAS library's first call loads its kernels)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        queue()                                             # (and its workspace on a stream that is not the default one)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    queue()
    t1.record()
    torch.cuda.synchronize()
    queue.ms = t0.elapsed_time(t1)
    print(f"\nlayers on streams: the delay ({DELAY_MATMULS} matmuls of {DELAY_N}^2 in fp32) takes {queue.ms:.1f} ms")
    yield queue
    del a, b, c


@pytest.fixture(scope="module")
def side(delay):
    """The side stream of Test 1.  The runtime maps its streams onto a few hardware queues (four by default), and a stream that shares the
    default stream's queue is ordered with it by the hardware: work on stream 0 then does wait for that stream's copies, and the test
    would see nothing.  So: the first of up to eight new streams on which the canary of Test 1 itself -- a NaN buffer, the delay and a
    copy into it queued on the stream, a clone taken on the default stream meanwhile -- still shows NaN.  Every case repeats the canary."""
    default = torch.cuda.default_stream()
    src = torch.zeros(4096, device="cuda")
    tried = []
    for _ in range(8):
        stream = torch.cuda.Stream()
        tried.append(stream)                                # (kept, so that the next one is another stream)
        buf = torch.full((4096,), NAN, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            delay()
            buf.copy_(src)
            with torch.cuda.stream(default):
                seen = buf.clone()
        torch.cuda.synchronize()
        if bool(torch.isnan(seen).any()):
            print(f"\nlayers on streams: side stream {len(tried)} of those tried runs beside the default stream")
            return stream
    pytest.fail("no stream runs beside the default stream: a clone on the default stream waited for the delay on each of eight new streams")


def test_the_table_is_the_one_named_here():
    assert [c.name for c in lc.cases()] == lc.NAMES
    assert [c.name for c in lc.cases() if not c.graph] == list(lc.OPTIMISERS)


@pytest.mark.parametrize("name", lc.NAMES)
def test_on_a_side_stream_whose_inputs_arrive_late(name, delay, side):
    case = _case(name)
    host = case.build(1)
    want = _eager(case, host)
    src = {k: v.cuda() for k, v in host.items()}
    ops = case.place(host)
    with torch.no_grad():
        for k in _buffers(host):
            ops[k].fill_(NAN)
    torch.cuda.synchronize()
    default = torch.cuda.default_stream()
    watched = ops[_buffers(host)[0]]
    with torch.cuda.stream(side):
        delay()
        _load(ops, src)
        with torch.cuda.stream(default):
            before = watched.clone()
        got = case.run(ops)
        with torch.cuda.stream(default):
            after = watched.clone()
    # (nothing on the default stream has waited for the side stream)
    side.synchronize()
    torch.cuda.synchronize()
    assert bool(torch.isnan(before).any()), (f"{name}: inconclusive -- the operand already held its values on the default stream when the call was "
                                             f"issued: the delay ({delay.ms:.1f} ms when measured) was over")
    assert bool(torch.isnan(after).any()), (f"{name}: the operand held its values on the default stream when the call had returned, and not when it "
                                            f"was issued: the call made the host wait for its stream (or took the rest of the {delay.ms:.1f} ms delay)")
    diff = _differing([t.detach() for t in got], want)
    assert not diff, f"{name} on a side stream: " + "; ".join(diff)


@pytest.mark.parametrize("name", [n for n in lc.NAMES if n not in lc.OPTIMISERS])
def test_captured_and_replayed_queued(name):
    case = _case(name)
    hosts = [case.build(1), case.build(2)]
    wants = [_eager(case, h) for h in hosts]
    assert _differing(wants[0], wants[1]), f"{name}: the two data sets give the same results"
    srcs = [{k: v.cuda() for k, v in h.items()} for h in hosts]
    static = case.place(hosts[0])
    _load(static, srcs[0])
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        case.run(static)                                    # the eager warm-up, on the capture stream
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):            # one linear chain: the case forks no stream
        outs = case.run(static)
    clones = []
    for i in range(REPLAYS):                                # B, A, B, A, B, A: queued, no host synchronisation in between
        _load(static, srcs[(i + 1) % 2])
        graph.replay()
        clones.append([t.detach().clone() for t in outs])
    torch.cuda.synchronize()
    failures = []
    for i, got in enumerate(clones):
        diff = _differing(got, wants[(i + 1) % 2])
        if diff:
            failures.append(f"replay {i} (data set {'AB'[(i + 1) % 2]}): " + "; ".join(diff))
    assert not failures, f"{name} captured and replayed: " + " | ".join(failures)


@pytest.mark.parametrize("batch", [1, 7, 39, 64])
def test_hyperbolic_loss_backward_has_the_bits_of_the_scalar_entry_point(batch):
    """gmath.hyperbolic_loss's backward divides the incoming gradient by the batch size on the device; hypad_hyper_loss_bwd takes it as a
    host float and divides there.  Same fp32 division, same kernel: same bits."""
    from hypad_amd import _C
    from hypad_amd.hyperspace import gmath
    host = _case("gmath.hyperbolic_loss").build(3)
    u, v, g = (host[k].cuda() for k in ("u", "v", "go"))
    ul, vl = u.clone().requires_grad_(True), v.clone().requires_grad_(True)
    got = torch.autograd.grad(gmath.hyperbolic_loss(ul, vl, batch), [ul, vl], g)
    gu, gv = torch.full_like(u, NAN), torch.full_like(v, NAN)
    _C.check(_C.lib.hypad_hyper_loss_bwd(_C.ptr(u), _C.ptr(v), float(g), _C.ptr(gu), _C.ptr(gv), u.shape[0], u.shape[1], batch, _C.stream()))
    torch.cuda.synchronize()
    assert torch.equal(got[0], gu) and torch.equal(got[1], gv)
