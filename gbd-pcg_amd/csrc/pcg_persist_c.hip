// pcg_persist_c.hip -- the persistent kernels (pcg_persist_kernels.hpp) of the block sizes 30 - 36; pcg_persist.hip dispatches here.
#include "pcg_persist_kernels.hpp"

namespace gbdpcg {
GBDPCG_PERSIST_GROUP(, 2)
}  // namespace gbdpcg
