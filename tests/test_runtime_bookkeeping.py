"""The host-side bookkeeping of ape_amd/runtime.py without a device: frame rows, the choice of a step's part, the ring of result
slots and its release, graph retirement with partial graphs, the lanes of a slot and their copy order, and the DMA helper's
handling of the environment.  Events and streams are stubs whose synchronize / wait / record do nothing."""
import contextlib
import itertools
import os

import pytest
import torch

from ape_amd import runtime
from ape_amd.runtime import _DmaTransfer, _Entry, _Slot, _frame_row, _lane_plan, _step_part

_SDMA_ENGINES_AT_IMPORT = os.environ.get("APE_SDMA_ENGINES")


class _Event:
    """stands in for torch.cuda.Event, torch.cuda.Stream and threading.Event"""

    def __init__(self, log=None, name=""):
        self.log, self.name = log, name

    def _note(self, what):
        if self.log is not None:
            self.log.append((what, self.name))

    def synchronize(self):
        self._note("synchronize")

    def wait(self, *a):
        self._note("wait")

    def wait_event(self, ev):
        self._note("wait_event:" + ev.name)

    def record(self, *a):
        self._note("record")


@pytest.fixture
def host_alloc(monkeypatch):
    """torch.empty / torch.zeros as the slot calls them, on the host: returns the log of (function, shape, pinned) requests"""
    log = []
    for fn in ("empty", "zeros"):
        def alloc(shape, dtype, device=None, pin_memory=False, _fn=fn, _real=getattr(torch, fn)):
            log.append((_fn, tuple(shape), bool(pin_memory)))
            return _real(shape, dtype=dtype)
        monkeypatch.setattr(torch, fn, alloc)
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    return log


def _slot(mask_format="bitmask", semantic=False, panoptic=False, with_masks=True):
    return _Slot(2, 5, 48, 7, "cpu", with_masks, mask_format, 16, semantic, panoptic)


@pytest.fixture
def sdma_env(monkeypatch):
    """_DmaTransfer's constructor writes APE_SDMA_ENGINES into the process's environment: start from an unset variable and put back
    whatever the session had (setenv first, so that an undo is recorded even when the variable was unset)"""
    for name in ("APE_SDMA_ENGINES", "APE_SDMA_MULTI"):
        monkeypatch.setenv(name, "placeholder")
        monkeypatch.delenv(name)
    monkeypatch.setattr(runtime.threading.Thread, "start", lambda self: None)


def test_frame_row():
    assert _frame_row((480, 640), (240, 320)) == [2, 2, 2, 2, 640, 480, 640, 480]
    row = _frame_row((480, 640), (240, 160))                   # non-square scale: x by 4, y by 2
    assert row == [4, 2, 4, 2, 640, 480, 640, 480] and row[0] != row[1]
    assert _frame_row((30, 50), (30, 50))[:4] == [1, 1, 1, 1]


def test_step_part():
    """pipelined with partial graphs: ViT only for the first step of a stream (no ticket completes), tails only for the flush (no
    images), the full step between; the full step everywhere else"""
    table = {(True, False): "vit", (True, True): "full", (False, True): "tails", (False, False): "tails"}
    for pipeline, partial in itertools.product((False, True), repeat=2):
        for (has_images, completes), part in table.items():
            want = part if pipeline and partial else "full"
            assert _step_part(pipeline, partial, has_images, completes) == want, (pipeline, partial, has_images, completes)


def _enqueue(entry):
    """what _replay does with a slot: claim it, and mark it busy once the step's results are on their way"""
    s = entry.claim_slot()
    s.busy = True
    return s


def test_slot_ring(host_alloc):
    assert runtime.GraphedForward.SLOTS == 2
    e = _Entry()
    e.slots = [_slot() for _ in range(runtime.GraphedForward.SLOTS)]
    assert not any(s.busy for s in e.slots)
    first, second = _enqueue(e), _enqueue(e)
    assert first is e.slots[0] and second is e.slots[1]
    with pytest.raises(RuntimeError, match="every result slot is outstanding"):
        e.claim_slot()
    first.wait()
    assert not first.busy and second.busy
    assert _enqueue(e) is first
    with pytest.raises(RuntimeError, match="every result slot is outstanding"):
        e.claim_slot()


def test_slot_is_released_when_its_transfer_failed(host_alloc):
    """the DMA helper's error is raised by wait() -- and the slot goes back to the ring (it stayed busy for ever before)"""
    e = _Entry()
    e.slots = [_slot(), _slot()]
    s = _enqueue(e)
    _enqueue(e)
    assert s.masks_done is None and s.masks_err is None and s.has_masks is False       # the constructor's state
    s.masks_done, s.masks_err = _Event(), [RuntimeError("ape_hip_sdma_d2h failed")]
    with pytest.raises(RuntimeError, match="ape_hip_sdma_d2h failed"):
        s.wait()
    assert s.busy is False
    assert e.claim_slot() is s


def test_retire_with_partial_graphs(monkeypatch):
    """a refused eviction parks NOTHING of an entry with partial graphs; an accepted one parks its three graphs and its bytes once"""
    monkeypatch.setattr(runtime, "_RETIRED", [])
    monkeypatch.setattr(runtime, "RETIRE_LIMIT_BYTES", 10 << 30)
    run = runtime.GraphedForward.__new__(runtime.GraphedForward)
    run._graphs, run.max_graphs = {}, 4
    entry = _Entry(graph=object(), graph_vit=object(), graph_tails=object(), pool_bytes=4 << 30)
    assert len(entry.graphs()) == 3 and _Entry(graph=object()).graphs() != [] and _Entry().graphs() == []
    run._retire(entry)
    assert runtime.retired_graphs() == (3, 4 << 30)
    assert {id(g) for g, _ in runtime._RETIRED} == {id(g) for g in entry.graphs()}
    run._retire(_Entry(graph=object(), graph_vit=object(), graph_tails=object(), pool_bytes=4 << 30))
    assert runtime.retired_graphs() == (6, 8 << 30)
    before = list(runtime._RETIRED)
    with pytest.raises(RuntimeError, match="any_size=True"):
        run._retire(_Entry(graph=object(), graph_vit=object(), graph_tails=object(), pool_bytes=4 << 30))
    assert runtime._RETIRED == before and runtime.retired_graphs() == (6, 8 << 30)
    run._retire(_Entry())                                      # an eager entry holds no graph
    assert runtime.retired_graphs() == (6, 8 << 30)


def test_entry_replays_the_full_step_without_partial_graphs():
    class Graph:
        replays = 0

        def replay(self):
            self.replays += 1

    full, vit, tails = Graph(), Graph(), Graph()
    e = _Entry(graph=full, graph_vit=vit, graph_tails=tails)
    e.outs, e.outs_tails = "outs", "outs_tails"
    assert [e.replay(p) for p in ("full", "vit", "tails")] == ["outs", "outs", "outs_tails"]
    assert (full.replays, vit.replays, tails.replays) == (1, 1, 1)
    e = _Entry(graph=full)
    e.outs = "outs"
    assert [e.replay(p) for p in ("full", "vit", "tails")] == ["outs"] * 3 and full.replays == 4


@pytest.mark.parametrize("mask_format,semantic,panoptic", list(itertools.product(("bitmask", "rle", "both"), (False, True), (False, True))))
def test_lane_table(host_alloc, mask_format, semantic, panoptic):
    B, k, maxpix, pq, cap = 2, 5, 48, 7, 16
    rle = mask_format in ("rle", "both")
    want = {"rec": ((B, k, 8), torch.float32, False)}
    if semantic:
        want["sem"] = ((B, maxpix), torch.int16, False)
    if panoptic:
        want["pan"] = ((B, maxpix), torch.int32, False)
        want["paninfo"] = ((B, pq + 1, 3), torch.int32, True)
    if rle:
        want["runs"] = ((B, k, cap), torch.int32, False)
        want["nruns"] = ((B, k), torch.int32, True)
    want["masks"] = ((B, k * maxpix), torch.uint8, False)
    plan = _lane_plan(B, k, maxpix, pq, True, mask_format, cap, semantic, panoptic)
    order = ["rec", "sem", "pan", "paninfo", "runs", "nruns", "masks"]
    assert [p[0] for p in plan] == [n for n in order if n in want]                     # the copy stream's order
    assert {n: (shape, dtype, zero) for n, shape, dtype, zero, _ in plan} == want
    assert {n for n, *_, host in plan if host} == set(want) - ({"masks"} if mask_format == "rle" else set())
    # without instance masks: no masks, no runs
    assert [p[0] for p in _lane_plan(B, k, maxpix, pq, False, mask_format, cap, semantic, panoptic)] == [n for n in order[:4] if n in want]
    # the constructor allocates exactly the plan: device half and pinned half of the same shape and dtype, zero-filled where planned
    s = _slot(mask_format, semantic, panoptic)
    assert [name for name, _, _ in s.lanes] == [p[0] for p in plan]
    for name in order:
        d, h = getattr(s, "d_" + name), getattr(s, "h_" + name)
        if name not in want:
            assert d is None and h is None
            continue
        shape, dtype, zero = want[name]
        assert tuple(d.shape) == shape and d.dtype == dtype
        assert (h is None) == (name == "masks" and mask_format == "rle")
        assert h is None or (tuple(h.shape) == shape and h.dtype == dtype)
        for half, pinned in ((d, False), (h, True)):
            if half is not None:
                assert ("zeros" if zero else "empty", shape, pinned) in host_alloc
    assert len(host_alloc) == sum(2 - (h is None) for _, _, h in s.lanes)
    assert (s.busy, s.has_masks, s.masks_done, s.masks_err) == (False, False, None, None)


class _Buf:
    """stands in for a tensor: `copy_` logs (destination, source), indexing logs nothing and names the part"""

    def __init__(self, log, name):
        self.log, self.name = log, name

    def __getitem__(self, index):
        b, part = index
        return _Buf(self.log, f"{self.name}[{b},:{part.stop}]")

    def copy_(self, src, non_blocking=False):
        assert non_blocking
        self.log.append(("copy", self.name, src.name))


@pytest.mark.parametrize("blit", [False, True])
def test_copy_out_order(host_alloc, monkeypatch, blit):
    """everything the copy stream gets, in order: wait(computed), one copy per lane in the lanes' order -- the masks only as a blit, per
    image and only the k * fh * fw bytes of its frame --, record(copied)"""
    monkeypatch.setattr(torch.cuda, "stream", lambda stream: contextlib.nullcontext())
    log = []
    s = _slot("both", True, True)
    s.lanes = [(name, _Buf(log, "d_" + name), _Buf(log, "h_" + name)) for name, _, _ in s.lanes]
    s.computed, s.copied = _Event(log, "computed"), _Event(log, "copied")
    s.has_masks = True
    frames, k = [(4, 6), (8, 6)], 5
    s.copy_out(_Event(log, "copy stream"), frames, k, blit_masks=blit)
    plain = [("copy", "h_" + n, "d_" + n) for n in ("rec", "sem", "pan", "paninfo", "runs", "nruns")]
    masks = [("copy", f"h_masks[{b},:{k * fh * fw}]", f"d_masks[{b},:{k * fh * fw}]") for b, (fh, fw) in enumerate(frames)]
    assert log == [("wait_event:computed", "copy stream")] + plain + (masks if blit else []) + [("record", "copied")]
    # a step that pasted no masks moves neither masks nor runs
    del log[:]
    s.has_masks = False
    s.copy_out(_Event(log, "copy stream"), frames, k, blit_masks=blit)
    assert log == [("wait_event:computed", "copy stream")] + plain[:4] + [("record", "copied")]
    # "rle": the masks have no host half, blit or not
    del log[:]
    s = _slot("rle")
    s.lanes = [(name, _Buf(log, "d_" + name), h if h is None else _Buf(log, "h_" + name)) for name, _, h in s.lanes]
    s.computed, s.copied, s.has_masks = _Event(log, "computed"), _Event(log, "copied"), True
    s.copy_out(_Event(log, "copy stream"), frames, k, blit_masks=blit)
    assert [entry[1] for entry in log[1:-1]] == ["h_rec", "h_runs", "h_nruns"]


def test_dma_helper_places_engines_on_the_constructing_thread(monkeypatch, sdma_env):
    d = _DmaTransfer(0)
    assert runtime.os.environ["APE_SDMA_ENGINES"] == "1" and d.one_by_one is False     # one process: engines placed
    monkeypatch.setenv("APE_SDMA_ENGINES", "3")                # an explicit setting wins
    monkeypatch.setenv("APE_SDMA_MULTI", "0")
    d = _DmaTransfer(0)
    assert runtime.os.environ["APE_SDMA_ENGINES"] == "3" and d.one_by_one is True


class _NoEnvironment:
    """a mapping whose every use fails"""

    def _refuse(self, *a, **k):
        raise AssertionError("the DMA helper thread touched the environment")

    __getitem__ = __setitem__ = __delitem__ = __contains__ = __iter__ = __len__ = _refuse
    get = setdefault = pop = keys = items = values = update = copy = _refuse


class _Lib:
    def __init__(self, status=0):
        self.calls, self.status = [], status

    def ape_hip_sdma_d2h(self, dst, src, n):
        self.calls.append(("one", dst, src, n))
        return self.status

    def ape_hip_sdma_d2h_multi(self, m, dsts, srcs, sizes, parts):
        self.calls.append(("multi", m, list(dsts), list(srcs), list(sizes), parts))
        return self.status

    def ape_hip_last_error(self):
        return b"copy engine said no"


@pytest.mark.parametrize("one_by_one", [False, True])
def test_dma_helper_thread_touches_no_environment(monkeypatch, sdma_env, one_by_one):
    import ape_amd._lib as _lib
    monkeypatch.setenv("APE_SDMA_MULTI", "0" if one_by_one else "1")
    d = _DmaTransfer(0)
    lib = _Lib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(torch.cuda, "set_device", lambda device: None)
    log = []
    done, err = d.submit(_Event(log, "computed"), [(0x1000, 0x2000, 30), (0x3000, 0x4000, 50)])
    d.close()
    with monkeypatch.context() as m:
        m.setattr(runtime.os, "environ", _NoEnvironment())
        d._run()                                               # the thread's body, here: one job, then the stop mark
    assert done.is_set() and err == [] and log == [("synchronize", "computed")]
    if one_by_one:
        assert lib.calls == [("one", 0x1000, 0x2000, 30), ("one", 0x3000, 0x4000, 50)]
    else:
        assert lib.calls == [("multi", 2, [0x1000, 0x3000], [0x2000, 0x4000], [30, 50], 0)]


def test_dma_helper_reports_a_failed_copy(monkeypatch, sdma_env):
    import ape_amd._lib as _lib
    d = _DmaTransfer(0)
    monkeypatch.setattr(_lib, "load", lambda: _Lib(status=1))
    monkeypatch.setattr(torch.cuda, "set_device", lambda device: None)
    done, err = d.submit(_Event(), [(0x1000, 0x2000, 30)])
    d.close()
    d._run()
    assert done.is_set() and len(err) == 1 and "copy engine said no" in str(err[0])


def test_dma_tests_leave_the_environment_as_it_was():
    """runs behind the tests above (file order): none of them left the engine placement set for later tests or their child processes"""
    assert os.environ.get("APE_SDMA_ENGINES") == _SDMA_ENGINES_AT_IMPORT
