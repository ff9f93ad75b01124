// explicit instantiations of the fused forward kernel families (SC supports x FPL features/lane)
#include "gml_spectconv_impl.h"
GML_FWD_FAMILY_SHAPES_D(GML_DEFINE_FWD_FAMILY)
