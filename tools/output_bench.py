#!/usr/bin/env python3
"""./output_bench.py [--gib 1] [--reps 5] - rates of the output calls (libsliceslice_hip_output.so), a measurement aid: one JSON
line per row, medians of `reps`, stream events around the calls, one process, one buffer, the routes taking turns.  The haystack
is the manual's text tiled to the size asked for, then the generator's bytes of the same size (ss.fill_random_device).  Rows:
  every line      the empty needle's records (every line) with line numbers: `format_lines` and `grep()` against
  descriptor -C 2 `descriptor` with two context lines on both sides, numbers and separators: the same
  one record      the bytes of `every line` (each line with its delimiter: the whole view) as ONE record - the balance case - beside
                  the same bytes gathered as lines
  generator       every line of the generator's bytes with line numbers
Per row:
  torch route     what tools/grep_hip.py does without --device-output: cumsum, `repeat_interleave` into an int64 index per output
                  byte, an index gather - with its host formatting loop left out (`torch_route_ms`) and, once, included
                  (`torch_route_with_host_loop_ms`: the copy to the host and the Python loop over the lines)
  ceiling         `torch` `copy_` of out_len contiguous bytes, and the plain-read ceiling (ss.read_ceiling_gbps)
  copy share      the share of the sized call spent in the copy pass: the sized call less the count-only call with d_starts (the size
                  passes and the starts)
  metadata        the bytes of records and starts the three passes read and write, beside the text bytes
Rows are printed as they come, those where the new call loses included."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sliceslice_rs_amd as ss  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def turns_ms(fns, reps):
    """medians of the device times of `fns`, taking turns"""
    times = [[] for _ in fns]
    for k in range(reps + 1):
        for j, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if k >= 1:
                times[j].append(a.elapsed_time(b))
    return [float(np.median(t)) for t in times]


def torch_route(hay, begin, end):
    length = end - begin
    start = torch.cumsum(length, 0) - length
    idx = torch.repeat_interleave(begin - start, length) + torch.arange(int(length.sum()), device=hay.device)
    return hay[idx], length


def host_loop(packed, length, number, kind):
    """the formatting loop of tools/grep_hip.py's context_lines"""
    packed = packed.cpu().numpy().tobytes()
    out, at, last = [], 0, None
    kinds = kind.cpu().tolist() if kind is not None else None
    for i, (n, ln) in enumerate(zip(number.cpu().tolist(), length.cpu().tolist())):
        if last is not None and n > last + 1:
            out.append(b"--\n")
        out.append(b"%d%s%s\n" % (n, b":" if kinds is None or kinds[i] else b"-", packed[at:at + ln]))
        at += ln
        last = n
    return b"".join(out)


def row(name, hay, records, separators, reps, ceiling, grep=None, with_host_loop=True):
    begin, end, number, kind = records
    count, n_bytes = begin.numel(), hay.numel()
    with ss.output_build():
        out = ss.format_lines(hay, begin, end, number, kind, separators=separators)
        out_len = out.numel()
        starts = torch.empty(count + 1, dtype=torch.int64, device="cuda")
        text_bytes = int((torch.clamp(end, max=n_bytes) - begin).sum())
        dst = torch.empty(out_len, dtype=torch.uint8, device="cuda")
        src = torch.empty(out_len, dtype=torch.uint8, device="cuda")
        fns = [lambda: ss.format_lines(hay, begin, end, number, kind, separators=separators),
               lambda: ss.format_lines_into(hay, begin, end, dst, number=number, kind=kind, separators=separators),
               lambda: ss.format_lines_into(hay, begin, end, None, number=number, kind=kind, separators=separators, d_starts=starts),
               lambda: torch_route(hay, begin, end), lambda: dst.copy_(src)] + ([grep] if grep else [])
        t = turns_ms(fns, reps)
        host_ms = None
        if with_host_loop:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            packed, length = torch_route(hay, begin, end)
            text = host_loop(packed, length, number, kind if separators else None)
            host_ms = (time.perf_counter() - t0) * 1e3
            assert len(text) == out_len and text[:4096] == out[:4096].cpu().numpy().tobytes()
            del packed, length, text
    records_bytes = count * (8 + 8 + 8 + (1 if kind is not None else 0))
    metadata = 3 * records_bytes + 2 * 8 * (count + 1)
    copy_ms = max(t[1] - t[2], 0.0)
    line = {"row": "output", "case": name, "gib": round(n_bytes / (1 << 30), 3), "records": count, "out_len": out_len, "text_bytes": text_bytes,
            "metadata_bytes": metadata, "metadata_over_text": round(metadata / max(text_bytes, 1), 3),
            "format_lines_ms": round(t[0], 3), "format_lines_into_ms": round(t[1], 3), "count_only_with_starts_ms": round(t[2], 3),
            "copy_pass_ms": round(copy_ms, 3), "copy_share_of_sized_call": round(copy_ms / t[1], 3),
            "copy_pass_gb_per_s": round(out_len / copy_ms / 1e6, 1) if copy_ms else None,
            "format_lines_into_gb_per_s": round(out_len / t[1] / 1e6, 1),
            "torch_route_ms": round(t[3], 3), "torch_route_over_format_lines": round(t[3] / t[0], 2),
            "torch_route_with_host_loop_ms": round(host_ms, 1) if host_ms is not None else None,
            "with_host_loop_over_format_lines": round(host_ms / t[0], 1) if host_ms is not None else None,
            "copy_ceiling_ms": round(t[4], 3), "copy_ceiling_gb_per_s": round(out_len / t[4] / 1e6, 1),
            "format_lines_into_over_copy_ceiling": round(t[1] / t[4], 2), "read_ceiling_gb_per_s": round(ceiling, 1),
            "format_lines_into_share_of_read_ceiling": round(out_len / t[1] / 1e6 / ceiling, 3), "reps": reps}
    if grep:
        line["grep_ms"] = round(t[5], 3)
    print(json.dumps(line), flush=True)
    del out, dst, src, starts
    torch.cuda.empty_cache()
    return line


def balance(hay, begin, end, reps):
    """the whole view as one record against the same bytes as lines (each with its delimiter, no terminator)"""
    n_bytes = hay.numel()
    b1, e1 = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), n_bytes, dtype=torch.int64, device="cuda")
    with_delimiter = end + 1
    dst = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    with ss.output_build():
        L = ss.lib()
        one = lambda: ss.searcher._format_into(L, hay, b1, e1, None, None, None, 0, dst, None, None, gather=True)                   # noqa: E731
        many = lambda: ss.searcher._format_into(L, hay, begin, with_delimiter, None, None, None, 0, dst, None, None, gather=True)   # noqa: E731
        assert one() == n_bytes and torch.equal(dst, hay)
        dst.zero_()
        assert many() == n_bytes and torch.equal(dst, hay)
        t = turns_ms([one, many, lambda: dst.copy_(hay)], reps)
    print(json.dumps({"row": "output", "case": "one record", "gib": round(n_bytes / (1 << 30), 3), "lines": begin.numel(),
                      "gather_one_record_ms": round(t[0], 3), "gather_as_lines_ms": round(t[1], 3), "one_record_over_lines": round(t[0] / t[1], 3),
                      "one_record_gb_per_s": round(n_bytes / t[0] / 1e6, 1), "as_lines_gb_per_s": round(n_bytes / t[1] / 1e6, 1),
                      "copy_ceiling_ms": round(t[2], 3), "copy_ceiling_gb_per_s": round(n_bytes / t[2] / 1e6, 1), "reps": reps}), flush=True)
    del dst
    torch.cuda.empty_cache()


def main():
    argv = sys.argv[1:]
    gib = float(argv[argv.index("--gib") + 1]) if "--gib" in argv else 1.0
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 5
    n_bytes = int(gib * (1 << 30))
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    hay = text.repeat(n_bytes // text.numel() + 1)[:n_bytes].contiguous()
    ceiling = ss.read_ceiling_gbps(hay)
    with ss.output_build():
        every, descriptor = ss.DynamicHipSearcher.new(b""), ss.DynamicHipSearcher.new(b"descriptor")
        begin, end, number = every.find_lines(hay)
        row("every line", hay, (begin, end, number, None), False, reps, ceiling, grep=lambda: every.grep(hay, line_numbers=True))
        balance(hay, begin, end, reps)
        del begin, end, number
        records = descriptor.find_lines_context(hay, 2, 2)
        row("descriptor -C 2", hay, records, True, reps, ceiling, grep=lambda: descriptor.grep(hay, 2, 2, line_numbers=True))
        del records
        ss.fill_random_device(hay, 0x5EED0001)
        begin, end, number = every.find_lines(hay)
        row("generator", hay, (begin, end, number, None), False, reps, ss.read_ceiling_gbps(hay), grep=lambda: every.grep(hay, line_numbers=True))


if __name__ == "__main__":
    main()
