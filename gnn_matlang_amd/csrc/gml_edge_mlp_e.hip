// explicit instantiations of the ML3Layer edge-branch kernels (S = Sout)
#include "gml_edge_mlp_impl.h"
GML_EMLP_S_E(GML_DEFINE_EDGE_MLP)
