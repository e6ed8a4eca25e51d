// ref-math-variant: <math.h> without libstdc++'s global float overloads.  <cmath> still declares the C library's
// double functions (sqrt, fabs, cos, ...) in the global namespace, so an unqualified call on a float argument in the
// reference promotes it to double (oracle/ASSUMPTIONS.md row 18).
#include <cmath>
