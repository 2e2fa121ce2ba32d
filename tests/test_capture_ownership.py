"""One owner for the engine's captured step: whatever invalidates a capture
(``set_batch_fn``, a layout switch, ``_check_lazy_moments`` turning the lazy rows off)
drops ALL of it through ``TrainEngine._drop_capture`` -- step graphs, K-step graph, the
hand-off counters that ``check_comm`` / ``comm_error`` consult, ``handoff_order`` --
and the next steps re-capture in the mode the configuration resolves to.

GPU: the data-parallel step (``force_segments``) of ONE engine, its collectives a
stand-in that needs no process group, in each of the step modes.  CPU: the same state
checks without graphs.
"""
import math
import warnings

import pytest
import torch

from ddim_cold_amd import build_model
from ddim_cold_amd.models import DiffusionVisionTransformer
from ddim_cold_amd.train.engine import EVENT_SPLIT, SEGMENTS, SINGLE, EngineConfig, TrainEngine

B = 8
TIMEOUT_US = 500_000


class _SelfComm:
    """A one-replica communicator: the sum over one rank, as a kernel on the caller's stream."""

    def all_reduce_(self, buf, op=0):
        buf.mul_(1.0)


def _batch(n, size, dev):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, 3, size, size, generator=g).clamp(-1, 1).to(dev)
    y = torch.randn(n, 3, size, size, generator=g).clamp(-1, 1).to(dev)
    t = torch.randint(1, 7, (n,), generator=g).to(dev)
    return x, y, t


def _dropped(eng):
    assert eng._graphs is None
    assert eng._multi is None
    assert eng.handoff_order is None
    assert eng._signal is None and eng._mode is None
    assert eng.comm_error() is False
    eng.check_comm()  # nothing to raise
    eng.reset_comm_error()


def _finite_steps(eng, n=2):
    for _ in range(n):
        loss = eng.train_step()
    assert math.isfinite(float(loss))


def _lazy_trigger(eng):
    """What a resumed optimizer state with moments on the never-selected rows does."""
    assert eng.lazy is not None
    eng.flat_m[eng.lazy[0]] = 1.0
    with pytest.warns(UserWarning, match="lazy weight decay off"):
        eng._check_lazy_moments()
    assert eng.lazy is None and eng._eager_steps == 0


# (layout, config, the layout apply_layout() switches to, mode, handoff_order)
CASES = {
    "event-split-overlap-2": ("overlap-2", {}, "inline-1", EVENT_SPLIT, "pre-issued"),
    "event-split-inline-1": ("inline-1", {}, "overlap-2", EVENT_SPLIT, "inline"),
    "captured": ("graph-overlap-2", dict(graph_steps=2), "graph-inline-1", SINGLE, None),  # + a 2-step graph
    "segments": (None, dict(comm_events=False, graph_comm=False), "overlap-4", SEGMENTS, None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_every_invalidation_drops_the_whole_capture(case, monkeypatch):
    monkeypatch.setenv("DDIM_COLD_HANDOFF_TIMEOUT_US", str(TIMEOUT_US))
    layout, extra, other, mode, order = CASES[case]
    torch.manual_seed(100)
    model = build_model("vit_tiny", drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0).cuda().train()
    eng = TrainEngine(model, EngineConfig(lr=1e-3, t_max=100, seed=5, temb_rows=7, graph_warmup=1,
                                          force_segments=True, **extra))
    eng.attach_comm(_SelfComm(), 1)
    if layout is not None:
        eng.apply_layout(layout)
    st = _batch(B, 64, "cuda")

    def fn():
        return st

    def captured(mode_, order_):
        torch.cuda.synchronize()
        assert eng._mode == mode_ and eng.handoff_order == order_
        assert len(eng._graphs) == {SINGLE: 1, EVENT_SPLIT: 2, SEGMENTS: len(eng.bucketing.bounds) + 1}[mode_]
        assert (eng._signal is not None) == (order_ in ("pre-issued", "post-replay"))
        assert not eng._graph_comm_failed
        assert (eng._multi is not None) == (mode_ == SINGLE and eng.cfg.graph_steps > 1)
        if eng._multi is not None:  # one replay of the K-step graph
            assert eng._multi[1] == eng.cfg.graph_steps
            assert math.isfinite(float(eng.train_steps(eng.cfg.graph_steps)))
        assert eng.comm_error() is False

    eng.set_batch_fn(fn)
    _finite_steps(eng, 3)  # warm-up, capture + replay, replay
    captured(mode, order)
    if eng._signal is not None:
        # an error word raised by the capture about to go must not outlive it
        eng._signal.err.fill_(1)
        assert eng.comm_error() is True

    eng.set_batch_fn(fn)  # no new warm-up: the next step captures
    _dropped(eng)
    _finite_steps(eng)
    captured(mode, order)

    eng.apply_layout(other)
    _dropped(eng)
    assert eng._eager_steps == 0
    _finite_steps(eng)  # warm-up, capture + replay
    captured(*{"inline-1": (EVENT_SPLIT, "inline"), "overlap-2": (EVENT_SPLIT, "pre-issued"),
               "overlap-4": (EVENT_SPLIT, "pre-issued"), "graph-inline-1": (SINGLE, None)}[other])

    _lazy_trigger(eng)
    _dropped(eng)
    _finite_steps(eng)
    assert eng._graphs is not None and eng.comm_error() is False
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", list(CASES))
def test_invalidations_leave_no_capture_state_cpu(case):
    layout, extra, other, _, _ = CASES[case]
    torch.manual_seed(0)
    model = DiffusionVisionTransformer(img_size=[16, 16], patch_size=4, embed_dim=32, depth=3, num_heads=2).train()
    eng = TrainEngine(model, EngineConfig(lr=1e-3, t_max=100, seed=5, temb_rows=7, graph_warmup=1, use_graph=False,
                                          force_segments=True, **extra), device="cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # graph- layouts: no capturable backend here
        if layout is not None:
            eng.apply_layout(layout)
        st = _batch(4, 16, "cpu")
        eng.set_batch_fn(lambda: st)
        _finite_steps(eng, 3)
        _dropped(eng)  # use_graph=False: never captured
        for trigger in (lambda: eng.set_batch_fn(lambda: st), lambda: eng.apply_layout(other)):
            trigger()
            _dropped(eng)
            _finite_steps(eng)
            _dropped(eng)
    _lazy_trigger(eng)
    _dropped(eng)
    _finite_steps(eng)
    _dropped(eng)
