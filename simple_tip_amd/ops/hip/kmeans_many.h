// Constants and launchers of the batched k-means kernels (kmeans_many.hip and
// the silhouette epilogue in pairwise.hip), shared with bindings.cpp. Plain
// C++.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

constexpr int KMEANS_MANY_MAX_PROBLEMS = 64;   // one wave lane per problem
constexpr int KMEANS_MANY_MAX_K = 16;          // centres per problem
constexpr int KMEANS_MANY_MAX_CENTERS = 256;   // stacked centres per call
// rows whose sums one block of the update folds before it writes a partial;
// a function of nothing, so the order of every sum depends on N alone
constexpr int KMEANS_MANY_CHUNK_ROWS = 256;

// labels / mind [P, N] from the squared distances d2 [N, C] to the stacked
// centres: per problem the minimum over its segment, ties to the lowest
// index, mind = sqrt(min).
void launch_lloyd_argmin(const float* d2, const int* seg, int n, int c, int p,
                         int* labels, float* mind, hipStream_t);

// One Lloyd update of every active problem. psum holds
// lloyd_chunks(n) * c * d floats, pshift c floats; counts [c] is zeroed here.
int lloyd_chunks(int n);
void launch_lloyd_update(const float* x, const int* labels, float* centers,
                         const int* seg, int* active, int n, int d, int p,
                         int c, double tol, float* psum, float* pshift,
                         int* counts, float* shift, hipStream_t);

// pairwise.hip
int silhouette_bins();
int silhouette_strips(int n);
void launch_silhouette_sums(const float* x, const float* xnorm, int n, int k,
                            const int* labels, const int* seg, int p0, int np,
                            int bin0, int nbins, int c, float* ppart,
                            float* out, hipStream_t);
