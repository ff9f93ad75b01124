// explicit instantiations of the matrix-core edge-branch kernels (S = Sout <= 8)
#include "gml_edge_chain_impl.h"
GML_ECHAIN_S_A(GML_DEFINE_EDGE_CHAIN)
