// Sample-list accessor of DDRotateInplaceTheory (see ref_peek.hpp).
#include <trajectory_generators/dd_rotate_inplace_theory.h>
#include "ref_peek.hpp"
REF_PEEK_DEFINE(rotate, trajectory_generators::DDRotateInplaceTheory)
