"""One line per point of the attention plan sweep, through ``torch.ops.ddim_cold.attn_keep_words``
(an op every build has): ``B H N hd -> words``.  Host only (no GPU).  The sweep is the one of
tests/cpp/attn_plan_check.cpp (B*H of 1, 4, 191, 192, 193 and 400, every N in 1..700 plus 1030,
2501 and 4096) over head dims 32 and 64 and two without kernels.  Comparing the output of two
builds (``DDIM_COLD_LIB=<other _C.so>``) shows whether a change moved the keep-word layout, and
so the path rule.  ``--plans``: the ``attn_plan`` lines instead (both directions, dropout and
keep buffer on and off), ``bwd B H N hd drop keep -> path hd np drop keep gx gy block lds
words`` or ``-> raises``.

usage: python tools/attn_plan_digest.py [--plans] [out.txt]     (prints the line count and a sha256)"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from ddim_cold_amd.ops import _ext

BHS = ((1, 1), (2, 2), (1, 191), (48, 4), (193, 1), (1, 400))
NS = tuple(range(1, 701)) + (1030, 2501, 4096)


def keep_word_lines():
    words = torch.ops.ddim_cold.attn_keep_words
    for hd in (32, 64, 16, 128):
        for B, H in BHS:
            for N in NS:
                yield f"{B} {H} {N} {hd} -> {int(words(B, H, N, hd))}"


def plan_lines():
    plan = torch.ops.ddim_cold.attn_plan
    for bwd in (False, True):
        for hd in (32, 64, 16):
            for drop in (False, True):
                for keep in (False, True):
                    for B, H in BHS:
                        for N in NS:
                            try:
                                got = " ".join(str(int(v)) for v in plan(bwd, B, H, N, hd, drop, keep))
                            except RuntimeError:
                                got = "raises"
                            yield f"{int(bwd)} {B} {H} {N} {hd} {int(drop)} {int(keep)} -> {got}"


def main():
    args = [a for a in sys.argv[1:] if a != "--plans"]
    plans = len(args) != len(sys.argv) - 1
    _ext.load(raise_on_error=True)
    h, n = hashlib.sha256(), 0
    out = open(args[0], "w") if args else None
    for line in (plan_lines() if plans else keep_word_lines()):
        h.update((line + "\n").encode())
        n += 1
        if out:
            out.write(line + "\n")
    if out:
        out.close()
    print(f"{n} {'plans' if plans else 'keep-word lines'}, sha256 {h.hexdigest()}")


if __name__ == "__main__":
    main()
