// The compact decision line of a cluster rule's window record: the first 128 bytes of the record hold,
// in 32-bit fields, everything the closed form of a run reads and most of what it writes.  This header is
// plain C++ (host and device), so the encoding and its fits-tests are tested on the CPU.
//   words  0..19  ten pairs (bucket number - base, PASS); a bucket word of all ones = no bucket (null)
//   words 20..21  base word: base bucket number (47 bits) and the flags below
//   words 22..23  threshold (the copy of SlotParam::thr, a double)
//   words 24..25  occupyCounter[PASS], occupyCounter[PASS_REQUEST]
//   words 26..31  cached counter group of one bucket (array order: WAITING, BLOCK, PASS_REQUEST,
//                 BLOCK_REQUEST, OCCUPIED_PASS, OCCUPIED_BLOCK)
// Bucket number = window start / windowLengthInMs.  A value that does not fit never gets clamped: the
// record turns wide (kLnWide), the 64-bit header behind the line takes over, and the line is ignored from
// then on except for that flag and the threshold copy.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SGA_LN_HD __host__ __device__ inline
#else
#define SGA_LN_HD inline
#endif

namespace sga {

constexpr int kLnPairs = 10;             // sampleCount up to this has a compact form
constexpr int kLnWords64 = 16;           // the line in int64 words (128 bytes)
constexpr int kLnBaseBits = 47;
constexpr uint64_t kLnBaseMask = (1ull << kLnBaseBits) - 1;
constexpr uint64_t kLnBaseSet = 1ull << 56;   // the base is chosen (a fresh record has none)
constexpr int kLnTagShift = 57;               // cache tag: index of the bucket the cached group belongs to
constexpr uint64_t kLnTagMask = 0xFull << kLnTagShift;
constexpr uint64_t kLnTagValid = 1ull << 61;
constexpr uint64_t kLnHasOcc = 1ull << 62;    // ClusterMetricLeapArray.hasOccupied
constexpr uint64_t kLnWide = 1ull << 63;
constexpr uint32_t kLnNoBucket = 0xFFFFFFFFu;
constexpr int64_t kLnMaxDelta = 0xFFFFFFFEll;  // largest bucket number - base
constexpr int64_t kLnMaxCount = 0xFFFFFFFFll;
// the base is put this many buckets before the first bucket written, so a clock that steps back a little
// finds its buckets representable
constexpr int64_t kLnBaseMargin = 1ll << 16;
static_assert(kLnPairs <= 16, "the tag's bucket index has four bits");
static_assert((kLnBaseMask & (kLnBaseSet | kLnTagMask | kLnTagValid | kLnHasOcc | kLnWide)) == 0 &&
                  (kLnBaseSet & kLnTagMask) == 0 && (kLnTagMask & kLnTagValid) == 0,
              "the flags lie above the base and do not overlap");
static_assert(2 * kLnPairs + 2 + 2 + 2 + 6 == 32, "the line is exactly 32 words");

enum : int { LN_BASE = 20, LN_THR = 22, LN_OCC = 24, LN_CACHE = 26 };

SGA_LN_HD bool ln_base_fits(int64_t q) { return q >= 0 && q <= (int64_t)kLnBaseMask; }
SGA_LN_HD int64_t ln_pick_base(int64_t q) { return q > kLnBaseMargin ? q - kLnBaseMargin : 0; }
SGA_LN_HD int64_t ln_base(uint64_t bw) { return (int64_t)(bw & kLnBaseMask); }
// bucket number q against a chosen base: representable as a 32-bit difference (all ones is taken)
SGA_LN_HD bool ln_delta_fits(int64_t q, int64_t base) {
    // q - base cannot overflow: base is below 2^47, q is a time in ms divided by a positive length
    return q >= base && q - base <= kLnMaxDelta;
}
SGA_LN_HD uint32_t ln_enc_delta(int64_t q, int64_t base) { return (uint32_t)(uint64_t)(q - base); }
SGA_LN_HD int64_t ln_dec_bucket(uint32_t d, int64_t base) { return base + (int64_t)d; }
SGA_LN_HD bool ln_count_fits(int64_t v) { return v >= 0 && v <= kLnMaxCount; }
SGA_LN_HD int ln_tag(uint64_t bw) { return (bw & kLnTagValid) ? (int)((bw & kLnTagMask) >> kLnTagShift) : -1; }
SGA_LN_HD uint64_t ln_with_tag(uint64_t bw, int j) {
    bw &= ~(kLnTagMask | kLnTagValid);
    return j < 0 ? bw : (bw | kLnTagValid | ((uint64_t)j << kLnTagShift));
}

}  // namespace sga
