// Sample-list accessor of DDSimpleTrajectoryGeneratorTheory (see ref_peek.hpp).
#include <trajectory_generators/dd_simple_trajectory_generator_theory.h>
#include "ref_peek.hpp"
REF_PEEK_DEFINE(dd, trajectory_generators::DDSimpleTrajectoryGeneratorTheory)
