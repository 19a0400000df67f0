// oracle/ref_shim: every header of the slice is the one file f3ds_ref_shim.h (see there)
#include "f3ds_ref_shim.h"
