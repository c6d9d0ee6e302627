// TEST INFRASTRUCTURE ONLY. Force-included (-include) into the draw-tape compiles of the reference's
// render_final_project.cpp and geometry.cpp (oracle/Makefile: _ref/libref_shade_tape_cr.so and its plain
// twin). <random> comes first, untouched; after it every `uniform_real_distribution` the reference names is
// the tape type below, whose operator() ignores the engine and hands out the next value of the tape that
// ref_tape_set (shade_harness.cpp) put in place. random_device and mt19937 stay the real ones: they are
// constructed and never consulted. The tape state is defined once, in the harness's translation unit.
#ifndef DT_REF_TAPE_RANDOM_H
#define DT_REF_TAPE_RANDOM_H
#ifdef __cplusplus
#include <random>

extern "C" {
extern const double* ref_tape_values;
extern int ref_tape_len;    // doubles on the tape
extern int ref_tape_pos;    // draws asked for so far, the ones past the end included
extern int ref_tape_over;   // 1 once a draw was asked for past the end (it got 0.5)
}

namespace std {
template <class T = double>
struct tape_real_distribution {
  tape_real_distribution() {}
  tape_real_distribution(T, T) {}
  template <class Engine>
  T operator()(Engine&)
  {
    const int i = ref_tape_pos++;
    if (i < ref_tape_len) return (T)ref_tape_values[i];
    ref_tape_over = 1;
    return (T)0.5;
  }
};
}  // namespace std

#define uniform_real_distribution tape_real_distribution
#endif
#endif
