// Sample-list accessor of OmniSimpleTrajectoryGeneratorTheory (see ref_peek.hpp).
#include <trajectory_generators/omni_simple_trajectory_generator_theory.h>
#include "ref_peek.hpp"
REF_PEEK_DEFINE(omni, trajectory_generators::OmniSimpleTrajectoryGeneratorTheory)
