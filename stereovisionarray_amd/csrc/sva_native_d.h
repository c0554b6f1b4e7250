// sva_native_d.h -- the native volume widths of Mode S.  Plain C++: the host
// argument checks (array_args.h) compile it without a HIP header.
#pragma once

namespace sva {

// Native volume width of a frame with D disparities: 64, 128, 192 or 256
// (the smallest >= D), 0 when D is outside 1..256.
inline int padded_D(int D) {
    return D <= 0 ? 0 : D <= 64 ? 64 : D <= 128 ? 128 : D <= 192 ? 192 : D <= 256 ? 256 : 0;
}

}  // namespace sva
