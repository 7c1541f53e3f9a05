#!/usr/bin/env python3
"""sha256 of each kernel inside a device listing (hipcc -S --cuda-device-only): the function's lines
from its label to its .Lfunc_end, plus its .amdhsa_kernel descriptor block.  For a file that gained
kernels: the ones that existed before can be compared one by one (profiles/signals_identity.log).

    python tools/kernel_listing_hash.py gte_backtest.s [more.s ...]
"""
import hashlib
import re
import sys


def kernel_hashes(text):
    out = []
    for m in re.finditer(r"^(_Z\w+):.*?^\.Lfunc_end\d+:\n", text, re.S | re.M):
        name = m.group(1)
        desc = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n.*?\.end_amdhsa_kernel\n", text, re.S)
        if desc is None:
            continue  # a device function, not a kernel
        out.append((name, hashlib.sha256((m.group(0) + desc.group(0)).encode()).hexdigest(), m.group(0).count("\n")))
    return out


if __name__ == "__main__":
    for path in sys.argv[1:]:
        for name, digest, lines in kernel_hashes(open(path).read()):
            print(f"{digest}  {name}  ({lines} lines)  {path}")
