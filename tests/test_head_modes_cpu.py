"""The head-step modes have one set of names and values: ``ops.HEAD_*`` in Python, ``enum HeadMode``
in csrc/kernels.h (read here as text: the op schemas pass plain ints, so no compiler compares them)."""
import os
import re

from ddim_cold_amd import ops

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(ops.__file__))), "csrc", "kernels.h")
SAMPLER_MODES = dict(HEAD_DDIM=1, HEAD_CLAMP=2, HEAD_DDIM_EACH=4, HEAD_ETA=5, HEAD_ETA_EACH=6)


def header_enum():
    with open(HEADER) as fh:
        body = re.search(r"enum HeadMode : int \{(.*?)\};", fh.read(), re.S).group(1)
    names = re.findall(r"^\s*(\w+) = (\d+),", body, re.M)
    assert len(names) == len(dict(names)), names
    return {k: int(v) for k, v in names}


def test_python_modes():
    got = {k: getattr(ops, k) for k in SAMPLER_MODES}
    assert got == SAMPLER_MODES and len(set(got.values())) == len(got)
    assert all(k in ops.__all__ for k in SAMPLER_MODES)


def test_header_enum_carries_the_same_values():
    assert header_enum() == dict(SAMPLER_MODES, HEAD_IMAGE=0, HEAD_LOSS=3)
    for k, v in header_enum().items():
        assert getattr(ops, k, v) == v, k
