// fields_launch.hpp - argument block, per-workgroup scratch records and host-side entry points of the field kernels
// (fields_kernels.hpp; defined and used in ss_fields.hip).
#pragma once
#include "runs_launch.hpp"

namespace ss {

constexpr int kFieldsSum = 0, kFieldsEmit = 1;                  // fields_kernel
constexpr int kFieldsCarryChunk = 256;                          // SS_FIELDS_CARRY_CHUNK: summaries per step of fields_carry_kernel

// FieldsSum::flags
constexpr uint32_t kFieldsVirtual = 1;      // the view's last byte lies in this workgroup and is no delimiter: the view's end closes a line
constexpr uint32_t kFieldsFirstIn = 2;      // MERGE: the workgroup's first byte is a field byte
constexpr uint32_t kFieldsLastIn = 4;       // MERGE: the last byte of the workgroup's 128 KiB is a field byte

// pass 1, one per workgroup.  The HEAD is the part in front of the workgroup's first delimiter (all of it where it has none).
struct FieldsSum {
    uint32_t nd;                // delimiters
    uint32_t head_events;       // events of the head
    uint32_t tail_events;       // events behind the last delimiter (nd != 0)
    uint32_t head_ends;         // MERGE: field ends of the head
    uint32_t begins, ends;      // record begins / ends that need no carry-in: those of the lines that begin inside the workgroup
    uint32_t flags;
    uint32_t reserved;
};

// the carry kernel's answer, one per workgroup
struct FieldsPre {
    uint64_t carry;             // events of the open line in front of the workgroup
    uint64_t lines;             // delimiters in front of the workgroup
    uint64_t rank_b, rank_e;    // record begins / ends in front of the workgroup
    uint32_t nb, ne;            // ... and inside it, the head line's included
    uint64_t reserved;
};

struct FieldsArgs {
    RunsArgs r;                 // the view; the set is the separators without the delimiter (EACH) or the field bytes (MERGE)
    uint64_t first, last;
    uint32_t merge, keep;
    uint32_t delim;
    FieldsSum *sum;             // pass 1: written
    const FieldsPre *pre;       // pass 2
    uint64_t *out_b, *out_e, *out_n;    // pass 2: each may be NULL; r.m.capacity records at most
};

struct FieldsCarryArgs {
    const FieldsSum *sum;
    FieldsPre *pre;
    uint64_t parts;
    uint64_t first, last;
    uint32_t merge, keep;
    uint64_t *totals;           // [0] record begins, [1] record ends, [2] lines
};

// ceil(ntiles / kSetTiles) workgroups of kBlock lanes
hipError_t launch_fields(const FieldsArgs &a, int mode, hipStream_t st);
// ONE workgroup of kFieldsCarryChunk lanes
hipError_t launch_fields_carry(const FieldsCarryArgs &a, hipStream_t st);

}  // namespace ss
