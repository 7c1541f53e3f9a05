// gte_hot.hip — the ONE instantiation the headline shape runs (classic step kernel, 16-byte
// vectors, cooperative phase A, raw rings staged in LDS), compiled alone in its own
// translation unit.  hipcc's code generation for a kernel depends on what is compiled next to
// it (builds of the same source differed by +-5 us per step); an isolated TU makes the hot
// kernel's code independent of every other kernel in the library.
//
// Compiled twice (gte_hot_body.h): here (sc1 observation stores: the observation buffer stays in the
// Infinity Cache, batches up to ~190 MB of observations) and in gte_hot_nt.hip
// (non-temporal stores: streaming, for bigger batches).
#define GTE_HOT_ONLY 1
#define GTE_HOT_NT 2
#define GTE_HOT_NAME(x) x
#include "gte_hot_body.h"
