"""The median-filter part of ``discorpy.prep`` on the GPU: see :mod:`discorpy_amd.prep.preprocessing`."""
