"""The calibration step of ``discorpy.proc`` (:mod:`discorpy_amd.proc.processing`): from grouped lines of points to the centre of
distortion, the radial coefficients and the perspective coefficients.  Host code (NumPy, SciPy): a few thousand numbers, once per lens."""
from . import processing  # noqa: F401
