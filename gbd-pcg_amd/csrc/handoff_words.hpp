// handoff_words.hpp -- the primitive types and constants of the tagged hand-off words that workgroups on different CUs pass
// each other inside one launch: shared by the persistent kernels (pcg_persist_handoff.hpp) and the cluster kernel
// (pcg_cluster_handoff.hpp), whose protocols differ in everything above this level.
#pragma once

namespace gbdpcg {

typedef unsigned long long u64;
// what the raw buffer builtins load and store: {value bits, tag} (8 bytes) or {low, tag, high, tag} (16 bytes)
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int kSc1 = 16;   // cache-policy bits of the raw buffer builtins on gfx94x/gfx950: bit 4 = sc1

}  // namespace gbdpcg
