// Stand-in at the include path the reference uses; see ref_pcl.hpp.
#include "../../ref_pcl.hpp"
