"""The Python binding, pinned call for call against tests/golden/engine_calls.json (recorded from the host forms of
tests/engine_calls.py): which library functions a method calls, with which scalars, arrays and variogram structures,
what it returns and what it refuses.  No kernel runs; the library is a stand-in that writes the calls down."""
import copy
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import engine_calls as EC  # noqa: E402


def _golden():
    return EC.load_golden()


def _diff(a, b, path=""):
    """Paths at which two JSON values differ (floats compare exactly: the binding does no arithmetic on them)."""
    if type(a) is not type(b):
        yield f"{path}: {a!r} != {b!r}"
    elif isinstance(a, dict):
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                yield f"{path}.{k}: only on one side"
            else:
                yield from _diff(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, list):
        if len(a) != len(b):
            yield f"{path}: {len(a)} entries != {len(b)}"
        for i, (x, y) in enumerate(zip(a, b)):
            yield from _diff(x, y, f"{path}[{i}]")
    elif a != b:
        yield f"{path}: {a!r} != {b!r}"


def test_host_calls_match_golden():
    golden = _golden()
    got = json.loads(json.dumps(EC.run_all()))
    assert sorted(got) == sorted(golden)
    bad = [d for name in sorted(golden) for d in _diff(golden[name], got[name], name)]
    assert not bad, "\n".join(bad[:40])


# Where the device form of a call legitimately differs from its host form, by entry point (the text before "[" of the
# case id), with the line of gss/engine.py at the commit the golden file was recorded on that establishes it.  The
# list is closed: a difference that is not here is a failure.
def _ndup_tensor(ret):
    ret = copy.deepcopy(ret)
    ret[4] = ["tensor", "int64", [1], "device"]
    return ret


def _second_stays(golden_ret, ret):
    ret = copy.deepcopy(ret)
    ret[2] = golden_ret[2]
    return ret


DEVICE_RETURNS = {
    # engine.py:1232 `return count, lagsum, zsum, (ndup if dev else int(ndup[0]))`: nduplicates stays a 1-element tensor
    "variogram_empirical": lambda g, r: _ndup_tensor(r),
    "variogram_plane": lambda g, r: _ndup_tensor(r),          # engine.py:1366, the same line
    "variogram_cross": lambda g, r: _ndup_tensor(r),          # engine.py:1426, the same line
    # engine.py:1282 `wmean = None if z is None else np.empty(s.shape[0])`: the per-size means are a host array
    "decluster_cells": _second_stays,
    # engine.py:102 `out = np.empty(tuple(t.shape), dtype=dt)`: a numpy copy is what to_host is for
    "to_host": lambda g, r: g,
}
# Host form accepted, device form refused: the arrays of the case then lie in two memory spaces.  (library call
# that the refusal comes before, exception type, message)
DEVICE_RAISES = {
    "variogram_empirical[mixed_spaces]": ("gss_variogram_empirical", "ValueError",
                                          "x and z must live in the same memory space"),                 # engine.py:1206
    "knn_search[mixed_spaces]": ("gss_knn_search", "ValueError",
                                 "xdata and centers must live in the same memory space"),                # engine.py:992
    "krig.predict_global_batch[mixed_spaces]": ("gss_krig_predict_global_batch", "ValueError",
                                                "xdom and zbatch must live in the same memory space"),   # engine.py:297
    "decluster_cells[mixed_spaces]": ("gss_decluster_cells", "ValueError",
                                      "x and z must live in the same memory space"),                     # engine.py:1270
    "fftgs.realize[noise_elsewhere]": ("gss_fftgs_realize", "ValueError",
                                       "noise and out must live in the same memory space"),              # engine.py:539
}


def _to_device(ret):
    if isinstance(ret, list):
        if ret[:1] == ["ndarray"]:
            return ["tensor", ret[1], ret[2], "device"]
        return [_to_device(e) for e in ret]
    return ret


def _strip(calls):
    """Calls without what the two forms differ in by construction: the array kind, its memory space, the flag."""
    calls = copy.deepcopy(calls)
    for _, args in calls:
        for a in args:
            if isinstance(a[1], dict):
                a[1].pop("kind"), a[1].pop("mem")
            if a[0] == "mem":
                a[1] = "mem"
    return calls


@pytest.mark.gpu
def test_device_calls_match_host_golden():
    golden = _golden()
    got = json.loads(json.dumps(EC.run_all(dev=True)))
    assert sorted(got) == sorted(n for n, host_only, _ in EC.cases() if not host_only)
    bad = []
    for name in sorted(got):
        g, d = golden[name], got[name]
        if name in DEVICE_RAISES:
            refused, *raised = DEVICE_RAISES[name]
            bad += list(_diff(raised, d.get("raised"), name + ".raised"))
            bad += list(_diff(_strip([c for c in g["calls"] if c[0] != refused]), _strip(d["calls"]), name + ".calls"))
            continue
        bad += list(_diff(_strip(g["calls"]), _strip(d["calls"]), name + ".calls"))
        for (fn, gargs), (_, dargs) in zip(g["calls"], d["calls"]):
            for ga, da in zip(gargs, dargs):
                if ga[0] == "mem" and (ga[1], da[1]) != (["int", 0], ["int", 1]):
                    bad.append(f"{name}.{fn}: mem {ga[1]} on the host, {da[1]} on the device")
        if "raised" in g:
            bad += list(_diff(g["raised"], d.get("raised"), name + ".raised"))
            continue
        want = _to_device(g["returned"])
        fix = DEVICE_RETURNS.get(name.split("[")[0])
        if fix is not None:
            want = fix(g["returned"], want)
        bad += list(_diff(want, d.get("returned"), name + ".returned"))
    assert not bad, "\n".join(bad[:40])
