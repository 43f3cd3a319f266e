// Launch arguments of the fused coverage suite (coverage_suite.hip), shared
// with bindings.cpp. Plain C++: the structs travel to the kernels by value.
#pragma once

#include <hip/hip_runtime.h>

constexpr int SUITE_MAX_LAYERS = 8;  // tapped layers per call
constexpr int SUITE_MAX_FAMILY = 4;  // profiles per family per call
constexpr int SUITE_MAX_SECTIONS = 16;  // a neuron's KMNC bits fit 16 bits
constexpr int SUITE_MAX_TOPK = 4;

// Threshold families. Profile slot = family * 4 + index, families in the
// order NAC, SNAC, NBC, KMNC; `scores` is [profiles, rows] in that order
// (inactive slots skipped), zero-initialised.
struct SuiteArgs {
  const float* layer[SUITE_MAX_LAYERS];  // [rows, width[l]] each
  int off[SUITE_MAX_LAYERS];    // first concatenated column; INT_MAX past L
  int width[SUITE_MAX_LAYERS];
  int rows, K;
  int n_nac, n_snac, n_nbc, n_kmnc;
  float nac_thr[SUITE_MAX_FAMILY];
  int kmnc_sec[SUITE_MAX_FAMILY];
  const float* snac_hi;   // [n_snac, K]
  const float* nbc_lo;    // [n_nbc, K]
  const float* nbc_hi;    // [n_nbc, K]
  const float* kmnc_lo;   // [K]
  const float* kmnc_hi;   // [K]
  unsigned long long* words[4 * SUITE_MAX_FAMILY];  // [rows, W(slot)]
  long long* scores;
};

// Top-k family: one top-4 per (row, layer) serves every requested k.
struct SuiteTopkArgs {
  const float* layer[SUITE_MAX_LAYERS];
  int off[SUITE_MAX_LAYERS];
  int width[SUITE_MAX_LAYERS];
  int rows, L, W, n;
  int k[SUITE_MAX_FAMILY];
  unsigned long long* words[SUITE_MAX_FAMILY];  // [rows, W], zeroed
  long long* scores[SUITE_MAX_FAMILY];          // [rows], zeroed
};

int coverage_suite_chunk();
void launch_coverage_suite_threshold(const SuiteArgs&, hipStream_t);
void launch_coverage_suite_topk(const SuiteTopkArgs&, hipStream_t);
