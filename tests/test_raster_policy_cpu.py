"""The rasterizer's deferred-check bookkeeping (gaussianip_amd/rasterizer.py), the parts that need no GPU: what the host
learns from a landed header, how an overflow is reported, and the ring of header slots.

A slip here costs silently truncated images and zero-gradient steps, not a crash, so the protocol is pinned on the host
alone: stand-in events, an ordinary tensor as the ring, no launch and no library."""
import warnings

import pytest
import torch

KEY = (0, 1000, 4, 256, 256)                  # device, P, V, H, W (rasterizer._hint_key)
BKEY = KEY + (False,)                         # + the list mode (rasterizer._bucket_key)


class _Event:
    """What the bookkeeping asks of a torch.cuda.Event."""

    def __init__(self, done):
        self.done, self.syncs = done, 0

    def query(self):
        return self.done

    def synchronize(self):
        self.syncs += 1


def _no_library():
    raise AssertionError("the bookkeeping reached for the HIP library")


@pytest.fixture
def R(monkeypatch):
    from gaussianip_amd import _lib
    from gaussianip_amd import rasterizer as R
    monkeypatch.setattr(_lib, "raster_lib", _no_library)
    monkeypatch.setattr(R, "_header_ring", torch.zeros((R._HEADER_SLOTS, 16), dtype=torch.int32))
    monkeypatch.setattr(R, "_header_next", 0)
    monkeypatch.setattr(R, "_header_owner", [None] * R._HEADER_SLOTS)
    monkeypatch.setattr(R, "_pending_checks", [])
    monkeypatch.setattr(R, "_capacity_hint", {})
    monkeypatch.setattr(R, "_bucket_hint", {})
    monkeypatch.setattr(R, "overflow_events", 0)
    monkeypatch.delenv("GIP_RASTER_ON_OVERFLOW", raising=False)
    assert R._HEADER_SLOTS == 64
    return R


def _defer(R, event, cap, stride, key=KEY, bkey=BKEY):
    """Takes the next slot of the ring and leaves a check pending on it, as a deferred forward does.  Returns the pending check,
    its header view and its slot."""
    slot, header = R._header_slot()
    p = R._Pending(event, header, slot, key, bkey, cap, stride)
    R._defer(p)
    return p, header, slot


def _land(header, num_rendered, overflow, max_tile):
    """The words the binning kernel mirrors into the slot (GipRasterHeader: capacity, num_rendered, overflow, max_tile_count)."""
    header[1], header[2], header[3] = num_rendered, overflow, max_tile


def _deferred(R, num_rendered, overflow, max_tile, cap, stride):
    """A deferred forward whose header has landed and whose event is complete: the next drain settles it."""
    ev = _Event(done=True)
    _, header, _ = _defer(R, ev, cap, stride)
    _land(header, num_rendered, overflow, max_tile)
    return ev


# ---------------------------------------------------------------------------------------------
# header digestion
# ---------------------------------------------------------------------------------------------
def test_a_landed_header_teaches_both_hints_without_a_warning(R):
    R._capacity_hint[KEY], R._bucket_hint[BKEY] = 5000, 300
    ev = _deferred(R, num_rendered=0, overflow=0, max_tile=17, cap=1 << 20, stride=672)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        R._drain_pending()
    assert R._capacity_hint[KEY] == 1                              # an empty frame: the hint stays a valid capacity
    assert R._bucket_hint[BKEY] == 300                             # a shorter longest list never lowers the bucket hint
    assert R.overflow_events == 0 and R._pending_checks == [] and ev.syncs == 0
    _deferred(R, num_rendered=4000, overflow=0, max_tile=301, cap=1 << 20, stride=672)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        R._drain_pending()
    assert R._capacity_hint[KEY] == 4000 and R._bucket_hint[BKEY] == 301      # the capacity hint follows the last call, the bucket hint rises
    assert R._pick_capacity(KEY) == max(R._MIN_CAPACITY, 3 * 4000 + R._CAPACITY_MARGIN)


def test_the_synchronous_reader_learns_the_same_and_reports_nothing(R):
    """The checked-now forward reads its header through the same function: it learns, and re-runs instead of reporting."""
    R._bucket_hint[BKEY] = 300
    header = torch.zeros(16, dtype=torch.int32)
    _land(header, 0, 0, 17)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert R._read_header(header, KEY, BKEY) == (0, False, 17)
        assert R._capacity_hint[KEY] == 1 and R._bucket_hint[BKEY] == 300
        _land(header, 70000, 1, 900)
        assert R._read_header(header, KEY, BKEY) == (70000, True, 900)
    assert R._capacity_hint[KEY] == 70000 and R._bucket_hint[BKEY] == 900 and R.overflow_events == 0


OVERFLOWS = {                                  # num_rendered  max_tile  cap   stride  message
    "dense": (2000, 700, 1000, 0, "2000 tile instances exceeded the capacity hint 1000"),
    "dense, within the capacity": (900, 700, 1000, 0, "900 tile instances exceeded the capacity hint 1000"),
    "bucketed, over the capacity": (2000, 97, 1000, 96, "2000 tile instances exceeded the capacity hint 1000"),
    "bucketed, only the list too long": (900, 97, 1000, 96, "a tile list of 97 entries outgrew its bucket of 96"),
}


@pytest.mark.parametrize("case", list(OVERFLOWS))
def test_an_overflow_is_counted_and_named(R, case):
    num_rendered, max_tile, cap, stride, message = OVERFLOWS[case]
    R._bucket_hint[BKEY] = 16
    _deferred(R, num_rendered, 1, max_tile, cap, stride)
    with pytest.warns(RuntimeWarning, match=message) as caught:
        R._drain_pending()
    assert len(caught) == 1 and "zero-gradient step" in str(caught[0].message)
    assert R.overflow_events == 1 and R._pending_checks == []
    assert R._capacity_hint[KEY] == num_rendered and R._bucket_hint[BKEY] == max_tile
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        R._drain_pending()                                         # reported once
    assert R.overflow_events == 1


@pytest.mark.parametrize("case", list(OVERFLOWS))
def test_an_overflow_raises_on_request(R, monkeypatch, case):
    num_rendered, max_tile, cap, stride, message = OVERFLOWS[case]
    monkeypatch.setenv("GIP_RASTER_ON_OVERFLOW", "raise")
    _deferred(R, num_rendered, 1, max_tile, cap, stride)
    with pytest.raises(RuntimeError, match=message + r".*\(GIP_RASTER_ON_OVERFLOW=raise\)"):
        R._drain_pending()
    assert R.overflow_events == 1 and R._pending_checks == []      # counted, taught and gone: the next call does not raise again
    assert R._capacity_hint[KEY] == num_rendered and R._bucket_hint[BKEY] == max_tile
    R._drain_pending()
    monkeypatch.delenv("GIP_RASTER_ON_OVERFLOW")
    _deferred(R, num_rendered, 0, max_tile, cap, stride)           # flag clear: nothing to raise or warn about
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        R._drain_pending()
    assert R.overflow_events == 1


# ---------------------------------------------------------------------------------------------
# the ring of header slots
# ---------------------------------------------------------------------------------------------
def test_ring_reuse_settles_the_unread_owner_once(R):
    """65 deferred forwards in a row, none of them complete: the 65th takes slot 0 again, whose first owner is synchronised,
    read and removed before the slot is handed out.  The other 63 stay pending until a blocking drain, which settles every
    remaining check once."""
    n = R._HEADER_SLOTS
    events, checks, keys = [], [], []
    for i in range(n):
        key = (0, 1000 + i, 4, 256, 256)
        events.append(_Event(done=False))
        p, header, slot = _defer(R, events[i], cap=1000, stride=0, key=key, bkey=key + (False,))
        assert slot == i
        _land(header, 5000 + i, 1, 40 + i)                         # every one overflowed: a settlement is an overflow event
        checks.append(p)
        keys.append(key)
    plan = R._Plan()
    plan.pending = checks[0]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        R._drain_pending()                                         # nothing has completed: nothing is settled
    assert len(R._pending_checks) == n and R.overflow_events == 0 and all(e.syncs == 0 for e in events)

    key = (0, 1000 + n, 4, 256, 256)
    events.append(_Event(done=False))
    with pytest.warns(RuntimeWarning, match="5000 tile instances exceeded the capacity hint 1000") as caught:
        p, header, slot = _defer(R, events[n], cap=1000, stride=0, key=key, bkey=key + (False,))
        # the first owner's words were read before the slot came back: the kernel may overwrite them now
        assert slot == 0 and R._capacity_hint[keys[0]] == 5000 and R._bucket_hint[keys[0] + (False,)] == 40
        _land(header, 5000 + n, 1, 40 + n)
    checks.append(p)
    keys.append(key)
    assert len(caught) == 1 and R.overflow_events == 1
    assert [e.syncs for e in events] == [1] + [0] * n
    assert len(R._pending_checks) == n and all(a is b for a, b in zip(R._pending_checks, checks[1:]))
    assert set(R._capacity_hint) == {keys[0]}                      # entries 2-64 and the newcomer are still unread

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        R._verify_pending(plan)                                    # its backward comes late: the ring has settled it already
        R._drain_pending()
    assert plan.pending is None and events[0].syncs == 1 and R.overflow_events == 1 and len(R._pending_checks) == n

    with pytest.warns(RuntimeWarning) as caught:
        R.settle_pending()
    assert len(caught) == n and R.overflow_events == n + 1 and R._pending_checks == []
    assert [e.syncs for e in events] == [1] * (n + 1)              # each waited for once, the first not again
    assert all(R._capacity_hint[k] == 5000 + i and R._bucket_hint[k + (False,)] == 40 + i for i, k in enumerate(keys))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        R.settle_pending()                                         # nothing is settled twice
    assert R.overflow_events == n + 1 and [e.syncs for e in events] == [1] * (n + 1)


def test_a_backward_settles_its_own_forward(R):
    """_verify_pending waits for the plan's event, settles its check and leaves the verdict on the plan; other checks stay."""
    other = _Event(done=False)
    _defer(R, other, cap=1000, stride=0)
    ev = _Event(done=False)
    plan = R._Plan()
    plan.pending, header, _ = _defer(R, ev, cap=1000, stride=96)
    _land(header, 900, 1, 97)
    with pytest.warns(RuntimeWarning, match="outgrew its bucket of 96"):
        R._verify_pending(plan)
    assert (plan.num_rendered, plan.overflowed, plan.pending) == (900, True, None)
    assert ev.syncs == 1 and other.syncs == 0 and len(R._pending_checks) == 1 and R.overflow_events == 1
