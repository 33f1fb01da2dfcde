"""gss -- host-side twin of GeoStatsSolvers.jl's KrigingSolver / FFTGS / LUGS over libgss_hip.so.

The package holds only what the hot path needs: the ctypes binding of the C-ABI (`_lib`), the
array-level engine (`engine`), the minimal geospatial containers the solvers read (`geo`), and the
solver front-ends (`solvers`) that mirror the reference's `solve(problem, solver)` API.
"""
from .geo import (CartesianGrid, Composition, DomainView, Ensemble, GeoTable, PointSet, SimpleMesh, aitchison, asarray,
                  domain, georef, parent, parentindices, triangulate, view)
from .problems import EstimationProblem, SimulationProblem
from .solvers import (FFTGS, LUGS, SGS, SPDEGS, CoKrigingSolver, CookieCutter, ExpWeight, IDWSolver, KrigingSolver,
                      LWRSolver, SPDEKriging, TricubeWeight, kriging_ui, searcher_ui, simulate_with_generic_loop, solve)
from .indicator import IndicatorKrigingSolver, SISSolver, postik
from .transforms import InNormalScores, NormalScore
from .validation import (BlockValidation, CrossValidationResult, KFoldValidation, LeaveBallOut, LeaveOneOut,
                         cross_validate, cverror)
from .variograms import (CubicVariogram, ExponentialVariogram, GaussianVariogram, MaternVariogram, MetricBall,
                         NestedVariogram, PentasphericalVariogram, PowerVariogram, SineHoleVariogram,
                         SphericalVariogram)
from .weighting import (BlockWeighting, CellDeclustering, PolygonalWeighting, Weights, weight, wmean, wquantile, wvar)
from .variography import (DirectionalVariogram, EmpiricalCrossVariogram, EmpiricalCrossVariogramResult,
                          EmpiricalVariogram, EmpiricalVariogramResult, EmpiricalVarioplane, EmpiricalVarioplaneResult,
                          LMCModel, fit, fit_anisotropic, fit_lmc)

__all__ = [n for n in dir() if not n.startswith("_")]
