// Accessors of the theories' protected sample list and cursor (see peek_*.cpp).
#ifndef REF_PEEK_HPP_
#define REF_PEEK_HPP_
#include <vector>
#include <Eigen/Core>
namespace trajectory_generators { class TrajectoryGeneratorTheory; }
#define REF_PEEK_DECL(tag)                                                                                       \
  std::vector<Eigen::Vector3f>& ref_peek_samples_##tag(trajectory_generators::TrajectoryGeneratorTheory& t);     \
  unsigned int& ref_peek_cursor_##tag(trajectory_generators::TrajectoryGeneratorTheory& t);
REF_PEEK_DECL(dd)
REF_PEEK_DECL(omni)
REF_PEEK_DECL(rotate)
// A pointer to a protected member taken through a derived class reads it without touching the reference's text.
#define REF_PEEK_DEFINE(tag, Theory)                                                                             \
  namespace {                                                                                                    \
  struct Peek : Theory {                                                                                         \
    static std::vector<Eigen::Vector3f> Theory::*samples() { return &Peek::sample_params_; }                    \
    static unsigned int Theory::*cursor() { return &Peek::next_sample_index_; }                                 \
  };                                                                                                             \
  }                                                                                                              \
  std::vector<Eigen::Vector3f>& ref_peek_samples_##tag(trajectory_generators::TrajectoryGeneratorTheory& t) {    \
    return static_cast<Theory&>(t).*Peek::samples();                                                             \
  }                                                                                                              \
  unsigned int& ref_peek_cursor_##tag(trajectory_generators::TrajectoryGeneratorTheory& t) {                     \
    return static_cast<Theory&>(t).*Peek::cursor();                                                              \
  }
#endif
