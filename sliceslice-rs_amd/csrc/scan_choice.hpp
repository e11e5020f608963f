// scan_choice.hpp - the kernel choice and the dynamic LDS size that the opt-in scans share (scan_inst_all.hip, scan_inst_lines.hip,
// scan_inst_nocase.hip; the product's own choice, with its search-only MODE 3 kernels, is scan_launch.hpp's).
#pragma once
#include <type_traits>

#include "scan_launch.hpp"

namespace ss {

// One needle slice per wave behind the padding that caps the workgroups resident per CU.
inline uint32_t scan_dyn_lds(const Shape &sh) { return sh.lds_pad + (sh.block / kWave) * kNeedleLds; }

template <int V>
using IntC = std::integral_constant<int, V>;

// Calls launch(Q, MODE, ONE_BYTE) - three std::integral_constant values - for the one of the nine kernels find() has that fits
// (q, mode, one_byte): one-byte needles take <0, 0, true>, a pair-alone searcher (mode 3) the MODE 2 kernel with its third byte.
// Returns false when no kernel fits (launch has not been called then).
template <class Launch>
bool choose_scan_kernel(int q, int mode, bool one_byte, Launch &&launch)
{
    if (one_byte) return launch(IntC<0>{}, IntC<0>{}, std::true_type{}), true;
    if (mode == 3) mode = 2;
    switch (q * 4 + mode) {
    case 0 * 4 + 0: return launch(IntC<0>{}, IntC<0>{}, std::false_type{}), true;
    case 0 * 4 + 2: return launch(IntC<0>{}, IntC<2>{}, std::false_type{}), true;
    case 1 * 4 + 0: return launch(IntC<1>{}, IntC<0>{}, std::false_type{}), true;
    case 1 * 4 + 2: return launch(IntC<1>{}, IntC<2>{}, std::false_type{}), true;
    case 2 * 4 + 0: return launch(IntC<2>{}, IntC<0>{}, std::false_type{}), true;
    case 2 * 4 + 2: return launch(IntC<2>{}, IntC<2>{}, std::false_type{}), true;
    case 3 * 4 + 0: return launch(IntC<3>{}, IntC<0>{}, std::false_type{}), true;
    case 3 * 4 + 2: return launch(IntC<3>{}, IntC<2>{}, std::false_type{}), true;
    }
    return false;
}

}  // namespace ss
