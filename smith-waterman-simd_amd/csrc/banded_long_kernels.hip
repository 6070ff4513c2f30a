// banded_long_kernels.hip -- the kernels of libswmi_banded_long.so (include/swmi_banded_long.h): the 32
// instantiations <K, kind, open >= extend, traceback> of banded_width_kernels.hip's sweep and walk for lengths up to 65536.
// The body is that file's text, compiled here a second time; its one block under SWMI_BANDED_LONG_KERNELS says what differs:
// the best cell's position packed as i << 10 | delta, and the diagonal clamped at +-131072.
#define SWMI_BANDED_LONG_KERNELS
#include "banded_width_kernels.hip"
