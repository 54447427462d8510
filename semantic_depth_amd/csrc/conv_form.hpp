// Which kernel runs a conv layer of a handle (DESIGN.md "which kernel runs a layer").  Host-side only: resolve_conv_form is the ONE place that walks the
// priority chain; capi.cpp keeps its results per handle and launches what a record names, sd_conv_forms prints the same records without a device.
#pragma once
#include <string>

#include "kernels.hpp"
#include "plan.hpp"

namespace sd {

struct HandleFacts { unsigned sw; int small_batch, cus; };     // what a handle fixes for the choice: switches, sd_set_small_batch level, the CU count its rules read

// CF_NONE: not a conv op, or nothing can run the layer (ConvForm::error).  CF_SPLITK / CF_DIRECT_SPLITC: the layer's reduce launch follows
enum ConvFamily : int { CF_NONE = 0, CF_IGEMM, CF_SPLIT, CF_STEM, CF_DMA, CF_DMA3, CF_SPLITK, CF_DIRECT, CF_DIRECT3, CF_DIRECT_SPLITC, CF_DEC_TAIL1 };

struct ConvForm {
    ConvFamily family = CF_NONE;
    int variant = 0;            // CF_DMA: block 1..5; CF_DMA3 / CF_SPLITK: gather mode 0..2; CF_SPLIT: tile 0..4 (conv_split.hip)
    bool s16 = false;           // CF_DMA3 / CF_SPLITK: 16x16x32 MFMAs (false: 32x32x16)
    DirectVariant direct{};     // CF_DIRECT / CF_DIRECT3
    int slices = 1;             // CF_SPLITK: slices of the K axis; CF_DIRECT_SPLITC: of the chunk axis
    int rowgrp = 0;             // CF_DMA3: ConvParams::rowgrp of a call whose image count is a multiple of it (run_plan; CALL-DEPENDENT)
    bool reads_images = false;  // the form depends on the image count of the call (CF_SPLIT with Cout % 256 == 0): a partial pass resolves it again
    ConvParams conv{};          // OP_CONV: the fields no call and no bound arena changes (N, rowgrp, alpha and every pointer are left to run_plan)
    ConvDirectParams dir{};     // OP_CONV_DIRECT: the same
    std::string label, verbose; // profile bucket of a plain run (bench.py groups by it); per-layer label of SEMDEPTH_PROFILE_VERBOSE and sd_conv_forms
    const char* error = nullptr;   // CF_NONE: the text run_plan fails with
};

// the form of one OP_CONV / OP_CONV_DIRECT / OP_DEC_TAIL1 op (any other: a default record) for a call of `images` images
ConvForm resolve_conv_form(const HandleFacts& hf, const NetPlan& p, const OpDesc& op, int images);

}  // namespace sd
