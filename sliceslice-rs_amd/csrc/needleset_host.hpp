// needleset_host.hpp - what a compiled needle set is on the host side: shared by ss_needleset.hip, which makes and frees it, and
// ss_setmatches.hip, which reads it (include/sliceslice_hip_needleset.h, include/sliceslice_hip_setmatches.h).
#pragma once
#include "ss_internal.hpp"

#include "needleset_tables.hpp"

struct ss_needle_set {
    ss::SetTables host;
    ss::SetView dev_view = {};
    uint8_t *d_mem = nullptr;
    int dev = -1;
    ss_searcher *anchor = nullptr;          // names the device and its scratch for ss_lines_around_device; its needle is never looked at
    ss::SetRanks dev_ranks = {};            // the side tables of needle identity, in the same allocation behind the blob
};
