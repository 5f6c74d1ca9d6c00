// pcg_persist_b.hip -- the persistent kernels (pcg_persist_kernels.hpp) of the block sizes 22 - 28; pcg_persist.hip dispatches here.
#include "pcg_persist_kernels.hpp"

namespace gbdpcg {
GBDPCG_PERSIST_GROUP(, 1)
}  // namespace gbdpcg
