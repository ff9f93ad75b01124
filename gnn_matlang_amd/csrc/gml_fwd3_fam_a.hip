// explicit instantiations of the 128-row forward kernel with the LDS-DMA landing ring, S = 8
#include "gml_spectconv_fwd3_impl.h"
GML_FWD3_SHAPES_A(GML_DEFINE_FWD3)
