#!/usr/bin/env python3
"""Fingerprint of what the IDW / LWR kernels return: a SHA-256 of the output bytes of every IDW / LWR case of
tests/search_cases.py (the est_*, idw_all_fast and lwr_all_fast entries, through HipEngine.idw / lwr) and of every case of
tests/test_gpu_est_cv.py::CASES (HipEngine.idw_cv / lwr_cv, with the lists and counts where the call returns them).

One JSON line per case on stdout: {"case", "sha256", "arrays"}.  Two builds of the library compute the same bytes iff
their listings are equal line for line; GSS_LIB_PATH selects the build:
    python tools/est_bytes.py > new.jsonl;  GSS_LIB_PATH=<other libgss_hip.so> python tools/est_bytes.py > other.jsonl"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import search_cases as SC  # noqa: E402
import search_matrix as SM  # noqa: E402
import test_gpu_est_cv as CV  # noqa: E402
import test_gpu_search_matrix as TM  # noqa: E402


def line(name, arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    print(json.dumps({"case": name, "sha256": h.hexdigest(), "arrays": len(arrays)}), flush=True)


def main():
    for key, case in SC.CASES.items():
        if key[0] in SC.EST_FAMILIES and isinstance(case, SC.Case):
            line(TM._id(key), TM._device_estimate(SM.problem_of(case), case))
    for c in CV.CASES:
        x, z, fold = CV.problem_of(c)
        line("cv-" + CV.ident(c), CV.device(c, x, z, fold, return_idx=c["k"] < c["n"]))


if __name__ == "__main__":
    main()
