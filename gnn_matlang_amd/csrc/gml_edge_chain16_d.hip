// explicit instantiations of the matrix-core edge-branch kernels for 8 < S = Sout <= 16
#include "gml_edge_chain16_impl.h"
GML_ECHAIN16_S_D(GML_DEFINE_EDGE_CHAIN16)
