// nocase_launch.hpp - host-side entry points of the case-folding scans (nocase_kernels.hpp; defined in scan_inst_nocase.hip, used
// by ss_nocase.hip).  Same arguments, kernel choice (scan_choice.hpp) and return value as launch_scan_all / launch_scan_lines.
#pragma once
#include "lines_launch.hpp"
#include "matches_launch.hpp"

namespace ss {

bool launch_scan_all_nocase(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const AllArgs &aa, uint32_t bound);
bool launch_scan_lines_nocase(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const LineArgs &la, uint32_t bound);

}  // namespace ss

struct ss_searcher;

namespace ssh {

// SS_OK when the searcher's needle holds no 'A'..'Z' (or s is NULL: the models' argument checks name that); else SS_ERR_ARGUMENT
// with the message that names ss_searcher_new_nocase.  `name` is the public function's.  (ss_nocase.hip)
int check_folded(const ss_searcher *s, const char *name);

}  // namespace ssh
