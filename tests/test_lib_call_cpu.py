"""The one host call path of the C-ABI (gaussianip_amd/_lib.py: ptr, call_model, call_nn, query_model) against a stub library, and a
scan of the package that keeps the by-hand protocol (`rc = lib.gip_X(..., stream)` / `raise RuntimeError("gip_X failed ...")`) from
coming back.  No GPU: the stub stands where the loaded library would, behind _lib._Counted."""
import ast
import contextlib
import ctypes
import pathlib

import pytest
import torch

from gaussianip_amd import _lib

PKG = pathlib.Path(_lib.__file__).resolve().parent
STREAM = 0x5EED0


class _Stub:
    """Entry points gip_ok / gip_query (status 0) and gip_bad (status 7); every call is recorded."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("gip_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            return 7 if name == "gip_bad" else 0
        return entry


@pytest.fixture
def stub(monkeypatch):
    s = _Stub()
    counted = _lib._Counted(s)
    monkeypatch.setattr(_lib, "_model", counted)
    monkeypatch.setattr(_lib, "_nn", counted)
    monkeypatch.setattr(_lib, "call_counts", {})
    s.streams_asked = []

    class _S:
        cuda_stream = STREAM

    def current_stream(dev=None):
        s.streams_asked.append(dev)
        return _S()
    monkeypatch.setattr(torch.cuda, "current_stream", current_stream)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())     # call_model selects dev: nothing to select here
    return s


@pytest.mark.parametrize("call", ["call_model", "call_nn"])
def test_call_passes_args_then_stream_counts_once_and_checks_the_status(stub, call):
    call = getattr(_lib, call)
    a, b = ctypes.c_void_p(16), ctypes.c_void_p(None)
    call("cuda:1", "gip_ok", a, 3, b, 2.5)
    (name, args), = stub.calls
    assert name == "gip_ok" and len(args) == 5
    assert args[0] is a and args[1] == 3 and args[2] is b and args[3] == 2.5
    assert isinstance(args[4], ctypes.c_void_p) and args[4].value == STREAM
    assert stub.streams_asked == ["cuda:1"]
    assert _lib.call_counts == {"gip_ok": 1}
    with pytest.raises(RuntimeError) as e:
        call("cuda:1", "gip_bad", a)
    assert "gip_bad" in str(e.value) and "status 7" in str(e.value) and "gip_ok" not in str(e.value)
    assert _lib.call_counts == {"gip_ok": 1, "gip_bad": 1}


def test_call_nn_hands_an_accepted_status_back(stub):
    assert _lib.call_nn("cuda:0", "gip_ok") == 0
    assert _lib.call_nn("cuda:0", "gip_bad", accept=(7,)) == 7
    with pytest.raises(RuntimeError):
        _lib.call_nn("cuda:0", "gip_bad", accept=(1,))


def test_query_model_appends_no_stream(stub):
    out = ctypes.c_size_t(0)
    ref = ctypes.byref(out)
    _lib.query_model("gip_query", 5, ref)
    assert stub.calls == [("gip_query", (5, ref))] and stub.streams_asked == []
    assert _lib.call_counts == {"gip_query": 1}
    with pytest.raises(RuntimeError) as e:
        _lib.query_model("gip_bad", 5)
    assert "gip_bad" in str(e.value) and "status 7" in str(e.value)
    assert stub.calls[-1] == ("gip_bad", (5,))


def test_ptr():
    assert _lib.ptr(None).value is None
    assert _lib.ptr(torch.empty(0)).value is None
    assert _lib.ptr(torch.empty((4, 0, 3))).value is None
    t = torch.arange(6.0)
    assert _lib.ptr(t).value == t.data_ptr() != 0
    assert _lib.ptr(t[2:]).value == t.data_ptr() + 2 * t.element_size()


def _modules():
    return sorted(p for p in PKG.rglob("*.py") if p.name not in ("_lib.py", "rasterizer.py"))


def _hand_launches(tree):
    """Calls of a `gip_` entry point as an attribute (lib.gip_X(...), getattr-free) that pass a `.cuda_stream` themselves."""
    names = {n.targets[0].id for n in ast.walk(tree) if isinstance(n, ast.Assign) and len(n.targets) == 1 and
             isinstance(n.targets[0], ast.Name) and "cuda_stream" in ast.unparse(n.value)}        # stream = c_void_p(... .cuda_stream)
    hits = []
    for n in ast.walk(tree):
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr.startswith("gip_"):
            for a in n.args:
                if "cuda_stream" in ast.unparse(a) or (isinstance(a, ast.Name) and a.id in names):
                    hits.append("%s at line %d" % (n.func.attr, n.lineno))
                    break
    return hits


def test_no_module_spells_the_call_protocol_by_hand():
    mods = _modules()
    assert len(mods) > 20 and any(p.name == "fused.py" for p in mods)
    bad = {}
    for p in mods:
        text = p.read_text()
        found = _hand_launches(ast.parse(text))
        if "failed with status" in text:
            found.append("a 'failed with status' message")
        if found:
            bad[str(p.relative_to(PKG))] = found
    assert not bad, "launch through _lib.call_model / call_nn / query_model instead: %s" % bad


def test_the_scan_sees_the_idiom():
    src = ("def f(x):\n"
           "    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)\n"
           "    rc = lib.gip_a(p(x), stream)\n"
           "    rc = _lib.nn_lib().gip_b(p(x), ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))\n"
           "    n = lib.gip_size(3)\n"
           "    key = (dev, torch.cuda.current_stream(dev).cuda_stream)\n")
    assert _hand_launches(ast.parse(src)) == ["gip_a at line 3", "gip_b at line 4"]
