"""The image-sized operations of ``discorpy.prep`` on the GPU: the median filter (:mod:`discorpy_amd.prep.preprocessing`) and the
Gaussian filter, the chessboard conversion and the tilted profile of the line-pattern route (:mod:`discorpy_amd.prep.linepattern`)."""
from . import linepattern, preprocessing  # noqa: F401
