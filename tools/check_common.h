// Host-side scaffolding the stand-alone check programs share (*_check.hip).  Each program
// keeps its own rnd() on top of rng_step(), since the ranges they draw from differ, and its
// own sentinels, mismatch reporter and cases.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

// the same bits: tells -0.0 from +0.0 and one NaN from another
static inline bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static inline uint64_t bits_of(double a) { uint64_t u; std::memcpy(&u, &a, 8); return u; }
static inline double from_bits(uint64_t u) { double d; std::memcpy(&d, &u, 8); return d; }

// one 64-bit linear congruential step: a program's draws, and so the counts in its PASS
// line, are the same on every run
[[maybe_unused]] static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static inline uint64_t rng_step() { return rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; }

// outputs start filled with this byte: a word that still holds it was not written
constexpr int kPoisonByte = 0xEE;
constexpr unsigned kPoison32 = 0xEEEEEEEEu;
constexpr uint64_t kPoison64 = 0xEEEEEEEEEEEEEEEEull;
static inline bool poisoned(const void* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (static_cast<const unsigned char*>(p)[i] != kPoisonByte) return false;
    return true;
}
