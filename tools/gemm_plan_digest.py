"""One line per point of the GEMM plan sweep, through ``torch.ops.ddim_cold.gemm_plan``
under each tile override: ``at bt epi override splits M N K -> dma bm bn waves stages``, or
``-> raises``.  Host only (no GPU).  The sweep is the one of tests/cpp/gemm_plan_check.cpp
(every built family, override -1..6, splits 1 / 2 / 4, sizes around every threshold) plus a
few (operand layout, epilogue) pairs no entry point launches.  Comparing the output of two
builds (``DDIM_COLD_LIB=<other _C.so>``) shows which plans a change moved.

usage: python tools/gemm_plan_digest.py [out.txt]     (prints the line count and a sha256)"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from ddim_cold_amd.ops import _ext

NT_EPIS = (0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 12)
FAMILIES = [(False, False, e) for e in NT_EPIS] + [(False, True, e) for e in (0, 1, 7)] + [(True, True, 8)]
# no gemm_nt / gemm_dgrad / gemm_wgrad call reaches these
UNBUILT = [(False, True, 3), (False, True, 2), (True, False, 0), (True, True, 1), (False, False, 8), (False, False, 9)]
MS = (1, 33, 300, 2080, 4160, 16383, 16384, 16448, 20032)
NS = (4, 64, 68, 192, 256, 384, 1152, 1536)
KS = (8, 48, 64, 128, 192, 384, 512, 576, 1152, 1536)


def lines():
    plan, override = torch.ops.ddim_cold.gemm_plan, torch.ops.ddim_cold.gemm_tile_override
    for at, bt, epi in FAMILIES + UNBUILT:
        for forced in range(-1, 7):
            prev = override(forced)
            try:
                for splits in (1, 2, 4):
                    for M in MS:
                        for N in NS:
                            for K in KS:
                                try:
                                    got = " ".join(str(int(v)) for v in plan(epi, at, bt, M, N, K, splits)[:5])
                                except RuntimeError:
                                    got = "raises"
                                yield f"{int(at)} {int(bt)} {epi} {forced} {splits} {M} {N} {K} -> {got}"
            finally:
                override(prev)


def main():
    _ext.load(raise_on_error=True)
    h, n = hashlib.sha256(), 0
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    for line in lines():
        h.update((line + "\n").encode())
        n += 1
        if out:
            out.write(line + "\n")
    if out:
        out.close()
    print(f"{n} plans, sha256 {h.hexdigest()}")


if __name__ == "__main__":
    main()
