#!/usr/bin/env python3
"""rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python tools/lines_trace.py MIB [CALLS]
CALLS (default 5) count_lines calls of `descriptor` over the manual's text tiled to MIB MiB, and nothing else from the lines
library: the kernel statistics of the run show what one call launches - one lines_scan_kernel plus the small launches - and how
long each takes at this size (tests/test_gpu_zz_lines_timing.py compares two sizes; profiles/lines/kernel_trace_summary.jsonl)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sliceslice_rs_amd as ss  # noqa: E402


def main():
    mib = int(sys.argv[1])
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    hay = torch.empty(mib << 20, dtype=torch.uint8, device="cuda")
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    hay.copy_(text.repeat(hay.numel() // text.numel() + 1)[:hay.numel()])
    with ss.lines_build():
        s = ss.DynamicHipSearcher(b"descriptor")
    for _ in range(calls):
        s.count_lines(hay)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
