"""Constants of the kernels, read from their source (the tests size their problems by the kernels' tiles and thresholds)."""
import os
import re

from conftest import ROOT

HEADERS = ("ba_kernels.hpp", "consumer_kernels.hpp")


def kernel_constant(name):
    """Value of `constexpr int <name> = <digits>;` in one of the kernel headers."""
    for header in HEADERS:
        src = open(os.path.join(ROOT, "sfm-python_amd", "csrc", header)).read()
        m = re.search(r"constexpr int %s = (\d+);" % name, src)
        if m:
            return int(m.group(1))
    raise KeyError(name)
