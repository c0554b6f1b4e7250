// sva_native_d.h -- the native volume widths of Mode S, and the launchers'
// instance ladders (a run-time class, integer or flag as a template argument).
// Plain C++: the host argument checks (array_args.h) and the aggregation plan
// (agg_plan.h) compile it without a HIP header.
#pragma once

#include <type_traits>

#include "sva_tuning.h"

namespace sva {

// Native volume width of a frame with D disparities: 64, 128, 192 or 256
// (the smallest >= D), 0 when D is outside 1..256.
inline int padded_D(int D) {
    return D <= 0 ? 0 : D <= 64 ? 64 : D <= 128 ? 128 : D <= 192 ? 192 : D <= 256 ? 256 : 0;
}

inline bool is_native_d(int D) { return D == 64 || D == 128 || D == 192 || D == 256; }

// What the aggregation kernels compile per native D: DPL disparities per lane
// (D / 16), the tile pipeline's log2 tile rows, and whether this class has the
// pair route (tune::kDiagPair*) and path minima (tune::kPathMinima*).
template <int DPL_, int TILE_LOG2, bool PAIR, bool MINIMA>
struct NativeD {
    static constexpr int DPL = DPL_, kTileLog2 = TILE_LOG2;
    static constexpr bool kPair = PAIR, kMinima = MINIMA;
};

// f(NativeD<..>{}) for the class of a native D; false, and no call, for any other D.
template <class F>
bool for_native_d(int D, F&& f) {
    constexpr int TL = tune::kWtahvTileLog2, TLW = tune::kWtahvTileLog2Wide;
    switch (D) {
        case 64: f(NativeD<4, TL, tune::kDiagPair4 != 0, tune::kPathMinima4 != 0>{}); return true;
        case 128: f(NativeD<8, TL, tune::kDiagPair8 != 0, tune::kPathMinima8 != 0>{}); return true;
        case 192: f(NativeD<12, TLW, tune::kDiagPair12 != 0, tune::kPathMinima12 != 0>{}); return true;
        case 256: f(NativeD<16, TLW, tune::kDiagPair16 != 0, tune::kPathMinima16 != 0>{}); return true;
        default: return false;
    }
}

// f(std::integral_constant<int, n>{}) for n in [Lo, Hi], one instance per value
// (instantiated from Lo up); false, and no call, for any other n.
template <int Lo, int Hi, class F>
bool for_int_in(int n, F&& f) {
    if constexpr (Lo > Hi) {
        return false;
    } else {
        if (n == Lo) {
            f(std::integral_constant<int, Lo>{});
            return true;
        }
        return for_int_in<Lo + 1, Hi>(n, f);
    }
}

// f(std::bool_constant<want && COMPILED>{}): a run-time flag as a template
// argument, where only the classes with COMPILED have the `true` instance.
template <bool COMPILED, class F>
void with_flag(bool want, F&& f) {
    if constexpr (COMPILED) {
        if (want) {
            f(std::true_type{});
            return;
        }
    }
    f(std::false_type{});
}

}  // namespace sva
