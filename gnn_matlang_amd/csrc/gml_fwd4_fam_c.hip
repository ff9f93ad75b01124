// chunked ring forward (gml_spectconv_fwd4_impl.h), S = 8: Fin <= 32 (groups beyond fwd3's staging: GML_FWD_CHUNKED)
#include "gml_spectconv_fwd4_impl.h"
GML_FWD4_SHAPES_C(GML_DEFINE_FWD4)
