/* TEST INFRASTRUCTURE ONLY. The float-libm rule DESIGN.md §5 declares for device and oracle: a float
 * transcendental is the double function of the widened argument, rounded once to float. Linked into
 * _ref/libref_shade_cr.so (oracle/Makefile, -Bsymbolic-functions) so that the reference's own calls of
 * these resolve here (sincosf too: at -O3 the compiler fuses a sinf / cosf pair of one argument into it); _ref/libref_shade.so is the same objects without this file. Compiled with
 * -fno-builtin: the bodies must call the double functions. */
#include <math.h>

float acosf(float x) { return (float)acos((double)x); }
float cosf(float x) { return (float)cos((double)x); }
float sinf(float x) { return (float)sin((double)x); }
float tanf(float x) { return (float)tan((double)x); }
float expf(float x) { return (float)exp((double)x); }
void sincosf(float x, float* s, float* c)
{
  *s = (float)sin((double)x);
  *c = (float)cos((double)x);
}
