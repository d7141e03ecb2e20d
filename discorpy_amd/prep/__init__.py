"""The image-sized operations of ``discorpy.prep`` on the GPU: the median filter (:mod:`discorpy_amd.prep.preprocessing`) and the
Gaussian filter, the chessboard conversion and the tilted profile of the line-pattern route (:mod:`discorpy_amd.prep.linepattern`), and
the sizes, axis ratios, slopes and lines of the dot-pattern route (:mod:`discorpy_amd.prep.dotpattern`)."""
from . import linepattern, preprocessing  # noqa: F401
from . import dotpattern  # noqa: F401
