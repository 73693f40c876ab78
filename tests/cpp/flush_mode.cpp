// Flush-to-zero and denormals-are-zero for the calling thread (x86-64 MXCSR bits 15 and 6): tests/test_levels_cpu.py sets them around a
// call of the CPU oracle to see what an implementation that flushes subnormals would answer on the level cases.  Returns the old state.
#include <xmmintrin.h>

extern "C" unsigned fx_test_flush_mode(unsigned on)
{
    const unsigned bits = 0x8040u, old = _mm_getcsr();
    _mm_setcsr(on ? (old | bits) : (old & ~bits));
    return (old & bits) == bits;
}
