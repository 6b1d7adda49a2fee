// blosc2_context.h -- what a blosc2_context holds here (private: shared by blosc2_shim.cpp and blosc2_getitem.cpp only).
#pragma once
#include "../../include/cimg_hip.h"

struct blosc2_context_s {
    bool compress;
    cimg_cparams cp;
    bool unsupported_params;     // prefilter / dict / non in-memory requests
};
