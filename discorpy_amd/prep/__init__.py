"""The image-sized operations of ``discorpy.prep`` on the GPU: the median filter (:mod:`discorpy_amd.prep.preprocessing`) and the
Gaussian filter, the chessboard conversion and the tilted profile of the line-pattern route (:mod:`discorpy_amd.prep.linepattern`), and
the sizes, axis ratios, slopes and lines of the dot-pattern route (:mod:`discorpy_amd.prep.dotpattern`), the sort and zoom behind
``calculate_threshold`` (:mod:`discorpy_amd.prep.threshold`), the point-list steps of strongly curved grids
(:mod:`discorpy_amd.prep.pointgrid`) and the module that carries every name of the reference's (:mod:`discorpy_amd.prep.complete`)."""
from . import linepattern, preprocessing  # noqa: F401
from . import dotpattern  # noqa: F401
from . import threshold, pointgrid, complete  # noqa: F401
