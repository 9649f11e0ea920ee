// The stable radix sorts of lattice_sort.hip.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace prg {

// Sorts n (key, value) pairs by the low `bits` bits of the key; equal keys keep their input order.  tmp == nullptr: only
// *tmp_bytes is set (workspace query).
int sort_pairs_u32(void* tmp, size_t* tmp_bytes, const unsigned* keys_in, unsigned* keys_out, const int* vals_in,
                   int* vals_out, unsigned n, unsigned bits, hipStream_t stream);
// The same for 64-bit keys (voxel.hip: the packed cell indices of the voxel grid).
int sort_pairs_u64(void* tmp, size_t* tmp_bytes, const uint64_t* keys_in, uint64_t* keys_out, const int* vals_in,
                   int* vals_out, unsigned n, unsigned bits, hipStream_t stream);

}  // namespace prg
