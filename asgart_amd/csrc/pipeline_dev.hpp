// pipeline_dev.hpp -- the device kernels of the probe -> search -> extend pipeline up to the extension, a file per stage
// over device_base.hpp; this file only lists them, in the order a call runs them:
//
//   probe_dev.hpp    the probe search: suffix-array interval and kept count of every probe
//   scan_dev.hpp     row offsets and segment starts, one pass over the counts
//   fill_dev.hpp     the hit rows
//   place_dev.hpp    the segments onto the extension tiers, the barren tests
//   ranges_dev.hpp   long segments cut into ranges that run side by side
// The extension kernels have a file each (extend_{wave,heavy,fast,k8}_dev.hpp) over extend_common_dev.hpp.
#pragma once

#include "probe_dev.hpp"
#include "scan_dev.hpp"
#include "fill_dev.hpp"
#include "place_dev.hpp"
#include "ranges_dev.hpp"
