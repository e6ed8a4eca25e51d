// Stand-in at the include path the reference uses; see ref_ros.hpp.
#include "../ref_ros.hpp"
