// bounded_how.hpp - the check of `how` that the bounded calls (ss_bounded.hip) and the inverted line calls (ss_inverted.hip) share:
// one set of refusals and messages (include/sliceslice_hip_bounded.h).
#pragma once
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_bounded.h"
#include "bounded_launch.hpp"
#include "nocase_launch.hpp"

namespace ssh {

// `how` and the needle of one call -> SS_OK and *bound, or the refusal.  line_form: a delimiter exists (checked by the models' code
// behind this; an invalid one never reaches a kernel).  unbounded_ok (the inverted line calls): neither SS_BOUND_WORD nor
// SS_BOUND_LINE is the plain or the folding scan, *bound = 0, and the empty needle is the models' then.
inline int check_how(const ss_searcher *s, unsigned how, bool line_form, int delimiter, const char *name, uint32_t *bound, bool unbounded_ok = false)
{
    const char *plain = line_form ? "ss_count_lines_device / ss_find_lines_device" : "ss_count_device / ss_find_all_device";
    const char *folding = line_form ? "ss_count_lines_nocase_device / ss_find_lines_nocase_device" : "ss_count_nocase_device / ss_find_all_nocase_device";
    if (how & ~(SS_BOUND_WORD | SS_BOUND_LINE | SS_BOUND_NOCASE))
        return fail(SS_ERR_ARGUMENT, "%s: how = 0x%x holds bits other than SS_BOUND_WORD | SS_BOUND_LINE | SS_BOUND_NOCASE", name, how);
    const bool word = (how & SS_BOUND_WORD) != 0, line = (how & SS_BOUND_LINE) != 0;
    if (!word && !line && !unbounded_ok)
        return fail(SS_ERR_ARGUMENT, "%s: how names neither SS_BOUND_WORD nor SS_BOUND_LINE; without a bound the call is %s", name,
                    (how & SS_BOUND_NOCASE) ? folding : plain);
    if (word && line)
        return fail(SS_ERR_ARGUMENT, "%s: how names both SS_BOUND_WORD and SS_BOUND_LINE; a call takes one of them", name);
    if (line && !line_form)
        return fail(SS_ERR_ARGUMENT, "%s: SS_BOUND_LINE needs lines; it belongs to ss_count_lines_bounded_device / ss_find_lines_bounded_device", name);
    if (s && s->n == 0 && (word || line))
        return fail(SS_ERR_ARGUMENT, "%s: the empty needle has no neighbour bytes to test (it is out of scope here)", name);
    if (how & SS_BOUND_NOCASE)
        if (int rc = check_folded(s, name)) return rc;
    *bound = !word && !line ? 0u : (word ? ss::kBoundWord : 0u) | (line_form ? ss::kBoundDelim | ((uint32_t)(delimiter & 0xFF) << ss::kBoundDelimShift) : 0u);
    return SS_OK;
}

}  // namespace ssh
