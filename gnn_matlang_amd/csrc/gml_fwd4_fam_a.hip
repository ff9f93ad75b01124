// chunked ring forward (gml_spectconv_fwd4_impl.h), S = 4: Fin <= 32 and Fin <= 48
#include "gml_spectconv_fwd4_impl.h"
GML_FWD4_SHAPES_A(GML_DEFINE_FWD4)
