// Stand-in at the include path the reference uses; see ref_tf2.hpp.
#include "../ref_tf2.hpp"
