"""Every compiled instantiation of the FFTGS kernels (tests/fftgs_cases.py) in the pipeline run that launches it: the
spectral amplitude, a seeded realisation and a realisation from supplied noise of every run against the 80-bit
restatement of fft.jl:96-103 and :163-170 (tests/fftgs_matrix.py), held to the bars of fftgs_cases.BARS -- 16 x the
error of the FP64 oracle against the same restatement, measured on the CPU, never on the device.  Co-simulations are
compared variable by variable with the mixture of the restatement's unit fields.

profiles/kernel_census_fftgs.txt is the kernel trace of this file alone: every kernel of the table launched at least
once."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fftgs_cases as FC
import fftgs_matrix as FM

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(FC.RUNS))
def test_run_matches_the_80_bit_restatement(name, monkeypatch):
    if not FM.long_double_ok():
        pytest.skip("numpy.longdouble is no finer than FP64 on this machine (eps %g): the 80-bit restatement of "
                    "tests/fftgs_matrix.py needs eps < 1e-18" % np.finfo(np.longdouble).eps)
    run = FC.RUNS[name]
    if run.path is None:
        monkeypatch.delenv("GSS_FFTGS_PATH", raising=False)
    else:
        monkeypatch.setenv("GSS_FFTGS_PATH", run.path)      # read by gss_fftgs_create
    got = FM.device_run(run)
    ref = FM.reference(run, FM.device_normals(run))
    e = FM.errors(got, ref)
    print("%s: F %.2e of max F (bar %.2e) at frequency %d   z %.2e (bar %.2e) at %s   scopes %s"
          % (name, e["F"][0], FC.BARS["F"]["bar"], e["F"][1], e["z"][0], FC.BARS["z"]["bar"], e["z"][1], got["scopes"]))
    # the pipeline the table says, and no other
    assert got["scopes"][run.pipeline] > 0 and not any(n for p, n in got["scopes"].items() if p != run.pipeline), got["scopes"]
    assert got["F"][0] == 0.0                                                   # fft.jl:103
    assert np.all(np.isfinite(got["F"])) and np.all(np.isfinite(got["z_seeded"])) and np.all(np.isfinite(got["z_noise"]))
    assert e["F"][0] <= FC.BARS["F"]["bar"], ("F", e["F"], FC.BARS["F"])
    assert e["z"][0] <= FC.BARS["z"]["bar"], ("z", e["z"], FC.BARS["z"])
