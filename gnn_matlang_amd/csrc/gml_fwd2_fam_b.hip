// explicit instantiations of the 128-row forward kernel, S = 12 (counting.py)
#include "gml_spectconv_fwd2_impl.h"
GML_FWD2_SHAPES_B(GML_DEFINE_FWD2)
GML_SPMM2_SHAPES_B(GML_DEFINE_SPMM2)
