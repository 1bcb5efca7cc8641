// smr_device.h -- device-side building blocks: element types, loads/stores with the
// StridedView `op` (identity/conj) applied, the fused elementwise functors and the
// wave-uniform f-program interpreter.  gfx950 only (wave64).
//
// Compiled with -ffp-contract=off: Julia never contracts (a+b)/2 or c*x+y into FMAs, and
// the map results must match the reference bit-for-bit for + - * / (SURVEY section 7).
#pragma once

#ifndef SMR_JIT
#include <hip/hip_runtime.h>
#endif

#include "smr_internal.h"

namespace smr {

#define SMR_DEV __device__ __forceinline__

// ---- device-side wall-clock stamps (debug build: make stamp -> libstrided_hip_stamp.so, -DSMR_STAMP=1) --------
// Profiler-independent timing of a launch: every wave records s_memrealtime (100 MHz, one clock for the whole
// device) at entry and after its last store has been acknowledged, into its own 16-byte slot of the region the
// launcher reserved for this launch (smr_set_option "stamp_base" / "stamp_cap" / "stamp_used"; tools/device_span.py
// turns the slots into first-start, last-end, cadence and inter-launch gap).  The product build compiles none of it.
#ifndef SMR_STAMP
#define SMR_STAMP 0
#endif
#if SMR_STAMP && !defined(SMR_JIT)
#define SMR_STAMP_PARAM , unsigned long long* smr_stamps
#define SMR_STAMP_ARG(grid, block) , ::smr::stamp_next((size_t)(grid) * (((size_t)(block) + 63) / 64))
#define SMR_STAMP_BEGIN const unsigned long long smr_t0 = (unsigned long long)wall_clock64();
#define SMR_STAMP_END ::smr::stamp_end(smr_stamps, smr_t0);
#else
#define SMR_STAMP_PARAM
#define SMR_STAMP_ARG(grid, block)
#define SMR_STAMP_BEGIN
#define SMR_STAMP_END
#endif
#if SMR_STAMP && !defined(SMR_JIT)
__device__ __forceinline__ void stamp_end(unsigned long long* stamps, unsigned long long t0) {
    if (!stamps) return;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long t1 = (unsigned long long)wall_clock64();
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* o = stamps + ((size_t)blockIdx.x * ((blockDim.x + 63) >> 6) + (threadIdx.x >> 6)) * 2;
        o[0] = t0;
        o[1] = t1;
    }
}
#endif

template <class R>
struct alignas(2 * sizeof(R)) cplx {
    R re, im;
};
typedef cplx<float> c32;
typedef cplx<double> c64;

// opaque movers for bit copies of 1- and 2-byte integers
struct b8 {
    uint8_t v;
};
struct b16 {
    uint16_t v;
};

template <class T> struct tr;
template <> struct tr<float> { typedef float real; static constexpr bool cx = false; static constexpr bool arith = true; static constexpr int dt = SMR_F32; };
template <> struct tr<double> { typedef double real; static constexpr bool cx = false; static constexpr bool arith = true; static constexpr int dt = SMR_F64; };
template <> struct tr<c32> { typedef float real; static constexpr bool cx = true; static constexpr bool arith = true; static constexpr int dt = SMR_C32; };
template <> struct tr<c64> { typedef double real; static constexpr bool cx = true; static constexpr bool arith = true; static constexpr int dt = SMR_C64; };
// the integer compute class: 64-bit two's-complement, wrapping (Julia's Int64 arithmetic); compiled with -fwrapv
typedef long long ix64;
template <> struct tr<ix64> { typedef ix64 real; static constexpr bool cx = false; static constexpr bool arith = true; static constexpr int dt = SMR_I64; };
template <> struct tr<b8> { typedef float real; static constexpr bool cx = false; static constexpr bool arith = false; static constexpr int dt = SMR_U8; };
template <> struct tr<b16> { typedef float real; static constexpr bool cx = false; static constexpr bool arith = false; static constexpr int dt = SMR_U16; };

// ---- construction / parts ----------------------------------------------------------------
// 16-/8-/4-byte vector store, plain or non-temporal.  A run-time switch between the two must not be written
// as if (nts) store_nt else store: the optimiser hoists/sinks the pair into ONE store and drops `nt`
// (seen in the ISA).  store_vec() keeps them apart with asm statements; loops over several stores
// branch once and bracket the non-temporal block with nt_block_guard().
// Store policy of a launch (kernel argument `nts`): 0 plain, 1 non-temporal, 2 agent-scope WRITE-THROUGH.
// Policy 2 ("self-released" launches, round 5): every store carries sc1 -- it is written through the XCD's L2 to the memory side, the
// level all eight XCDs share -- and the wave waits for the acknowledgements before it ends (self_release_wait).  When such a kernel
// has completed, nothing it wrote sits dirty in an L2: the release fence of its dispatch packet (a write-back of all eight L2s by the
// packet processor) has nothing left to do, and a recorded sequence drops it (smr_seq.cpp).  A later reader still acquires.
template <bool NT, class VT>
SMR_DEV void store_vec_ct(char* p, const VT& v) {
    // (the vector types carry 4-byte alignment: callers may hand in element-aligned addresses -- STREAM's UVec -- and the hardware
    // takes dwordx2 / dwordx4 accesses at any dword address; the instruction selected is the same)
    if constexpr (NT && sizeof(VT) == 16) {
        typedef uint32_t u4a __attribute__((ext_vector_type(4), aligned(4)));
        __builtin_nontemporal_store(*reinterpret_cast<const u4a*>(&v), reinterpret_cast<u4a*>(p));
    } else if constexpr (NT && sizeof(VT) == 8) {
        typedef uint32_t u2a __attribute__((ext_vector_type(2), aligned(4)));
        __builtin_nontemporal_store(*reinterpret_cast<const u2a*>(&v), reinterpret_cast<u2a*>(p));
    } else if constexpr (NT && sizeof(VT) == 4) {
        __builtin_nontemporal_store(*reinterpret_cast<const uint32_t*>(&v), reinterpret_cast<uint32_t*>(p));
    } else {
        *reinterpret_cast<VT*>(p) = v;
    }
}
// is there a write-through form for this vector type?  (launchers offer policy 2 only where every store of the kernel has one)
template <class VT>
struct has_wt_store {
    static constexpr bool value = sizeof(VT) == 16 || sizeof(VT) == 8 || sizeof(VT) == 4;
};
template <class VT>
SMR_DEV void store_vec_wt(char* p, const VT& v) {
    if constexpr (sizeof(VT) == 16) {
        typedef uint32_t u4 __attribute__((ext_vector_type(4)));
        const u4 x = *reinterpret_cast<const u4*>(&v);
        // The s_nop belongs to the store: on gfx940+ a VALU instruction that writes a data VGPR of a store of more than 64 bits needs
        // two wait states behind it (the store is still reading the register).  For its own stores the compiler inserts them; an
        // inline-asm statement is opaque to its hazard recogniser, and the register allocator does reuse the data registers for the
        // next address right away (seen in the ISA: wrong sums until the s_nop was added).
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(x) : "memory");
    } else if constexpr (sizeof(VT) == 8) {
        typedef uint32_t u2 __attribute__((ext_vector_type(2)));
        const u2 x = *reinterpret_cast<const u2*>(&v);
        asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(p), "v"(x) : "memory");
    } else if constexpr (sizeof(VT) == 4) {
        const uint32_t x = *reinterpret_cast<const uint32_t*>(&v);
        asm volatile("global_store_dword %0, %1, off sc1" ::"v"(p), "v"(x) : "memory");
    } else {
        *reinterpret_cast<VT*>(p) = v;  // (never offered: has_wt_store)
    }
}
// every store of this wave has been acknowledged by the memory side (policy 2: the last thing a wave does)
SMR_DEV void self_release_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
SMR_DEV void nt_block_guard() { asm volatile("; nt stores" ::: "memory"); }

// vector load, plain or non-temporal by a compile-time switch (a run-time switch belongs around the whole loop:
// a diamond per load is folded like the stores, and guarding each one keeps the loads of a batch apart)
template <int I>
struct IntC {
    static constexpr int value = I;
};
template <bool B>
struct BoolC {
    static constexpr bool value = B;
};
template <bool NT, class VT>
SMR_DEV VT load_vec_ct(const void* p) {
    if constexpr (NT && sizeof(VT) == 16) {
        typedef uint32_t u4 __attribute__((ext_vector_type(4)));
        VT v;
        *reinterpret_cast<u4*>(&v) = __builtin_nontemporal_load(reinterpret_cast<const u4*>(p));
        return v;
    } else {
        return *reinterpret_cast<const VT*>(p);
    }
}

template <class VT>
SMR_DEV void store_vec(char* p, const VT& v, int nts) {
    if (nts == 2) {
        store_vec_wt<VT>(p, v);
    } else if (nts) {
        nt_block_guard();
        store_vec_ct<true>(p, v);
        nt_block_guard();
    } else {
        store_vec_ct<false>(p, v);
    }
}

template <class T> struct is_int_class { static constexpr bool value = false; };
template <> struct is_int_class<ix64> { static constexpr bool value = true; };
// double -> the real type of a compute class; saturating for the integer class (the +-Inf seeds of min / max
// reductions become typemax / typemin, as _init_reduction! would give them)
template <class R> SMR_DEV R rcast(double d) { return R(d); }
template <> SMR_DEV ix64 rcast<ix64>(double d) {
    return d >= 9223372036854775807.0 ? 9223372036854775807LL : (d <= -9223372036854775808.0 ? (-9223372036854775807LL - 1) : (ix64)d);
}
template <class T> SMR_DEV T mk(typename tr<T>::real re, typename tr<T>::real im);
template <> SMR_DEV ix64 mk<ix64>(ix64 re, ix64) { return re; }
template <> SMR_DEV float mk<float>(float re, float) { return re; }
template <> SMR_DEV double mk<double>(double re, double) { return re; }
template <> SMR_DEV c32 mk<c32>(float re, float im) { return c32{re, im}; }
template <> SMR_DEV c64 mk<c64>(double re, double im) { return c64{re, im}; }

SMR_DEV float re_(float x) { return x; }
SMR_DEV double re_(double x) { return x; }
template <class R> SMR_DEV R re_(cplx<R> x) { return x.re; }
SMR_DEV ix64 re_(ix64 x) { return x; }
SMR_DEV ix64 im_(ix64) { return 0; }
SMR_DEV ix64 cj(ix64 x) { return x; }
SMR_DEV float im_(float) { return 0.f; }
SMR_DEV double im_(double) { return 0.; }
template <class R> SMR_DEV R im_(cplx<R> x) { return x.im; }

SMR_DEV float cj(float x) { return x; }
SMR_DEV double cj(double x) { return x; }
template <class R> SMR_DEV cplx<R> cj(cplx<R> x) { return cplx<R>{x.re, -x.im}; }
SMR_DEV b8 cj(b8 x) { return x; }
SMR_DEV b16 cj(b16 x) { return x; }

// ---- arithmetic (complex: Julia's plain 4-multiply product, Base complex.jl) -------------
template <class R> SMR_DEV cplx<R> operator+(cplx<R> a, cplx<R> b) { return cplx<R>{a.re + b.re, a.im + b.im}; }
template <class R> SMR_DEV cplx<R> operator-(cplx<R> a, cplx<R> b) { return cplx<R>{a.re - b.re, a.im - b.im}; }
template <class R> SMR_DEV cplx<R> operator-(cplx<R> a) { return cplx<R>{-a.re, -a.im}; }
template <class R> SMR_DEV cplx<R> operator*(cplx<R> a, cplx<R> b) {
    return cplx<R>{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
// The ends of the range, per real type: a complex value whose larger part is >= big or < small is multiplied by a power of two
// before hypot(x, y) + |x|, x*x + y*y or Smith's denominator is formed from it, and the result is scaled back (exact steps).
//   big    hypot and b.re + b.im * r stay finite below it (2 * sqrt(2) * big < floatmax)
//   small  above it nothing formed from the parts is subnormal; up = 4^upq brings every subnormal above it
template <class R> struct cxlim;
template <> struct cxlim<float> {
    static constexpr float big = 0x1p124f, small = 0x1p-100f, up = 0x1p48f, up_sqrt_inv = 0x1p-24f, up_inv = 0x1p-48f, up_log2 = 48.f;
    static constexpr float tanh_one = 22.5f;   // Base: 4|x| > asinh(floatmax): tanh(x + iy) is 1 to the last bit
};
template <> struct cxlim<double> {
    static constexpr double big = 0x1p1020, small = 0x1p-900, up = 0x1p108, up_sqrt_inv = 0x1p-54, up_inv = 0x1p-108, up_log2 = 108.;
    static constexpr double tanh_one = 177.75;
};
// 1/4, 1 or `up`: the factor that brings the larger part of (x, y) away from the ends of the range
template <class R> SMR_DEV R mid_scale(R x, R y) {
    const R m = fmax(fabs(x), fabs(y));
    return m >= cxlim<R>::big ? R(0.25) : (m < cxlim<R>::small ? cxlim<R>::up : R(1));
}
// Smith's division: avoids overflow of |b|^2
template <class R> SMR_DEV cplx<R> div_smith(cplx<R> a, cplx<R> b) {
    if (fabs(b.re) >= fabs(b.im)) {
        R r = b.im / b.re, den = b.re + b.im * r;
        return cplx<R>{(a.re + a.im * r) / den, (a.im - a.re * r) / den};
    } else {
        R r = b.re / b.im, den = b.re * r + b.im;
        return cplx<R>{(a.re * r + a.im) / den, (a.im * r - a.re) / den};
    }
}
template <class R> SMR_DEV cplx<R> operator/(cplx<R> a, cplx<R> b) {
    // Smith's division of operands that are scaled first where they lie at the ends of the range, each by its own power of two
    // (Base's inv(::ComplexF64) does it for the divisor), so that neither the denominator nor a numerator overflows or goes
    // subnormal where the quotient is representable; in the middle of the range (sa = sb = 1) every step is what it was
    const R sa = mid_scale(a.re, a.im), sb = mid_scale(b.re, b.im);
    a.re *= sa; a.im *= sa; b.re *= sb; b.im *= sb;
    cplx<R> q = div_smith(a, b);
    if (sa != sb) {  // q * (sb / sa), a power of two
        const R back = sb * (sa == R(1) ? R(1) : (sa < R(1) ? R(4) : cxlim<R>::up_inv));
        q.re *= back; q.im *= back;
    }
    return q;
}

template <class T> struct mathx;  // unary / binary ops of the f-program per compute type

template <class R>
struct mathx_real {
    static SMR_DEV R un(int op, R a) {
        switch (op) {
            case SMR_OP_NEG: return -a;
            case SMR_OP_ABS: return fabs(a);
            case SMR_OP_ABS2: return a * a;
            case SMR_OP_CONJ: return a;
            case SMR_OP_REAL: return a;
            case SMR_OP_IMAG: return R(0);
            case SMR_OP_SQRT: return sqrt(a);
            case SMR_OP_EXP: return exp(a);
            case SMR_OP_LOG: return log(a);
            case SMR_OP_SIN: return sin(a);
            case SMR_OP_COS: return cos(a);
            case SMR_OP_TANH: return tanh(a);
            case SMR_OP_INV: return R(1) / a;
            case SMR_OP_ROUND32: return (R)(float)a;
        }
        return a;
    }
    static SMR_DEV R bin(int op, R a, R b) {
        switch (op) {
            case SMR_OP_ADD: return a + b;
            case SMR_OP_SUB: return a - b;
            case SMR_OP_MUL: return a * b;
            case SMR_OP_DIV: return a / b;
            // Julia's min / max (Base/math.jl): NaN if either argument is NaN; min(-0.0, 0.0) = -0.0, max(-0.0, 0.0) = 0.0
            case SMR_OP_MIN: return (a != a) ? a : ((b != b) ? b : ((b < a) ? b : ((a < b) ? a : (__builtin_signbit(a) ? a : b))));
            case SMR_OP_MAX: return (a != a) ? a : ((b != b) ? b : ((a < b) ? b : ((b < a) ? a : (__builtin_signbit(a) ? b : a))));
            case SMR_OP_LT: return a < b ? R(1) : R(0);
            case SMR_OP_LE: return a <= b ? R(1) : R(0);
            case SMR_OP_GT: return a > b ? R(1) : R(0);
            case SMR_OP_GE: return a >= b ? R(1) : R(0);
            case SMR_OP_EQ: return a == b ? R(1) : R(0);
            case SMR_OP_NE: return a != b ? R(1) : R(0);
        }
        return a;
    }
    static SMR_DEV bool truthy(R a) { return a != R(0); }

    // The math opcodes (strided_hip.h: 65, 96..127, 128..159).  Runtime-compiled kernels only: FJit calls them with the opcode and
    // the exponent as template arguments, the interpreter never does (its switch stays as small as it is, csrc/smr_canon.cpp refuses
    // to interpret such a program).  Float32 calls the Float32 entry points of the device math library.
    template <int N>
    static SMR_DEV R powi(R a) {
        if constexpr (N == 0) return R(1);
        else if constexpr (N == 1) return a;
        else if constexpr (N == 2) return a * a;
        else if constexpr (N == 3) return a * a * a;
        else if constexpr (N == -1) return R(1) / a;
        else if constexpr (N == -2) { const R i = R(1) / a; return i * i; }
        else return (R)::powi((double)a, N);  // Julia: Float32 ^ n in Float64, rounded once; Float64: pown (within 1 ulp)
    }
    static SMR_DEV R fma3(R a, R b, R c) { return fma(a, b, c); }
    template <int OP>
    static SMR_DEV R ext_un(R a) {
        // Float32 asin, atan and log10 of the device library miss both neighbours of the exact value on some arguments (by one step:
        // tests/test_gpu_fprog_conformance.py); the Float64 function rounded once never does
        if constexpr (sizeof(R) == 4 && (OP == SMR_OP_ASIN || OP == SMR_OP_ATAN || OP == SMR_OP_LOG10))
            return (R)mathx_real<double>::template ext_un<OP>((double)a);
        // expm1(x) and log1p(x) are x -+ x^2/2...: below 2^-54 (2^-25) x itself is a neighbour of the exact value.  The library returns
        // +0.0 for -0.0 and flushes subnormal arguments.
        else if constexpr (OP == SMR_OP_EXPM1 || OP == SMR_OP_LOG1P) {
            if (fabs(a) < (sizeof(R) == 8 ? R(0x1p-54) : R(0x1p-25))) return a;
            if constexpr (OP == SMR_OP_EXPM1) return expm1(a);
            else return log1p(a);
        }
        else if constexpr (OP == SMR_OP_TAN) return tan(a);
        else if constexpr (OP == SMR_OP_ASIN) return asin(a);
        else if constexpr (OP == SMR_OP_ACOS) return acos(a);
        else if constexpr (OP == SMR_OP_ATAN) return atan(a);
        else if constexpr (OP == SMR_OP_SINH) return sinh(a);
        else if constexpr (OP == SMR_OP_COSH) return cosh(a);
        else if constexpr (OP == SMR_OP_EXP2) return exp2(a);
        else if constexpr (OP == SMR_OP_EXPM1) return expm1(a);
        else if constexpr (OP == SMR_OP_LOG2) return log2(a);
        else if constexpr (OP == SMR_OP_LOG10) return log10(a);
        else if constexpr (OP == SMR_OP_LOG1P) return log1p(a);
        else if constexpr (OP == SMR_OP_CBRT) return cbrt(a);
        else if constexpr (OP == SMR_OP_FLOOR) return floor(a);
        else if constexpr (OP == SMR_OP_CEIL) return ceil(a);
        else if constexpr (OP == SMR_OP_TRUNC) return trunc(a);
        else if constexpr (OP == SMR_OP_ROUND) return rint(a);  // round-to-nearest-even mode: Julia's RoundNearest
        else if constexpr (OP == SMR_OP_SIGN) return (a == R(0) || a != a) ? a : copysign(R(1), a);
        else if constexpr (OP == SMR_OP_NOT) return (R)(~(ix64)a);
        else return a;
    }
    template <int OP>
    static SMR_DEV R ext_bin(R a, R b) {
        if constexpr (OP == SMR_OP_POW) return pow(a, b);
        else if constexpr (OP == SMR_OP_ATAN2) return atan2(a, b);
        else if constexpr (OP == SMR_OP_HYPOT) {
            if constexpr (sizeof(R) == 4) {  // the squares are exact in Float64 and cannot overflow: two roundings there, one to Float32
                const double x = a, y = b;   // (the Float32 entry point misses both neighbours of the exact value on some arguments)
                const R h = (R)sqrt(x * x + y * y);
                return (fabs(a) == __builtin_huge_valf() || fabs(b) == __builtin_huge_valf()) ? (R)__builtin_huge_valf() : h;
            } else return hypot(a, b);
        }
        else if constexpr (OP == SMR_OP_REM) return fmod(a, b);
        else if constexpr (OP == SMR_OP_MOD) {  // Julia's mod(::T, ::T) for floats: floored, the result takes the sign of b
            const R r = fmod(a, b);
            if (r == R(0)) return copysign(r, b);
            return ((r > R(0)) != (b > R(0))) ? r + b : r;
        }
        else if constexpr (OP == SMR_OP_AND) return (R)((ix64)a & (ix64)b);
        else if constexpr (OP == SMR_OP_OR) return (R)((ix64)a | (ix64)b);
        else if constexpr (OP == SMR_OP_XOR) return (R)((ix64)a ^ (ix64)b);
        else return a;
    }
};
template <> struct mathx<float> : mathx_real<float> {};
template <> struct mathx<double> : mathx_real<double> {};

// integer class: every operation is closed over Int64 and wraps (unsigned arithmetic underneath: no UB);
// the planner admits only these opcodes (csrc/smr_canon.cpp: canonicalise)
template <> struct mathx<ix64> {
    typedef unsigned long long U;
    static SMR_DEV ix64 un(int op, ix64 a) {
        switch (op) {
            case SMR_OP_NEG: return (ix64)(U(0) - (U)a);
            case SMR_OP_ABS: return a < 0 ? (ix64)(U(0) - (U)a) : a;  // abs(typemin) = typemin, like Julia
            case SMR_OP_ABS2: return (ix64)((U)a * (U)a);
            case SMR_OP_IMAG: return 0;
            // Julia's narrow integer types, where their wrapping would be observed (inserted by the planner, csrc/smr_canon.cpp)
            case SMR_OP_WRAP_I8: return (ix64)(signed char)a;
            case SMR_OP_WRAP_I16: return (ix64)(short)a;
            case SMR_OP_WRAP_I32: return (ix64)(int)a;
            case SMR_OP_WRAP_U8: return a & 0xff;
            case SMR_OP_WRAP_U16: return a & 0xffff;
            case SMR_OP_WRAP_U32: return a & 0xffffffffLL;
        }
        return a;  // conj, real, round32 / widen (never emitted for integers)
    }
    static SMR_DEV ix64 bin(int op, ix64 a, ix64 b) {
        switch (op) {
            case SMR_OP_ADD: return (ix64)((U)a + (U)b);
            case SMR_OP_SUB: return (ix64)((U)a - (U)b);
            case SMR_OP_MUL: return (ix64)((U)a * (U)b);
            case SMR_OP_DIV: return b == 0 ? 0 : ((a == (-9223372036854775807LL - 1) && b == -1) ? a : a / b);  // not admitted by the planner (Julia's `/` leaves the integers)
            case SMR_OP_MIN: return b < a ? b : a;
            case SMR_OP_MAX: return a < b ? b : a;
            case SMR_OP_LT: return a < b ? 1 : 0;
            case SMR_OP_LE: return a <= b ? 1 : 0;
            case SMR_OP_GT: return a > b ? 1 : 0;
            case SMR_OP_GE: return a >= b ? 1 : 0;
            case SMR_OP_EQ: return a == b ? 1 : 0;
            case SMR_OP_NE: return a != b ? 1 : 0;
        }
        return a;
    }
    static SMR_DEV bool truthy(ix64 a) { return a != 0; }

    // math opcodes (runtime-compiled kernels only); the planner admits x ^ n for n >= 0, floor / ceil / trunc / round (identities),
    // sign, ~, & | xor, fma (= a*b + c) and rem / mod by a non-zero constant
    template <int N>
    static SMR_DEV ix64 powi(ix64 a) {
        U r = 1, x = (U)a;
        for (int n = N < 0 ? 0 : N; n > 0; n >>= 1) {  // the product mod 2^64 does not depend on its order
            if (n & 1) r *= x;
            x *= x;
        }
        return (ix64)r;
    }
    static SMR_DEV ix64 fma3(ix64 a, ix64 b, ix64 c) { return (ix64)((U)a * (U)b + (U)c); }
    template <int OP>
    static SMR_DEV ix64 ext_un(ix64 a) {
        if constexpr (OP == SMR_OP_SIGN) return a > 0 ? 1 : (a < 0 ? -1 : 0);
        else if constexpr (OP == SMR_OP_NOT) return ~a;
        else return a;  // floor ceil trunc round: identities on integers
    }
    template <int OP>
    static SMR_DEV ix64 ext_bin(ix64 a, ix64 b) {
        if constexpr (OP == SMR_OP_REM || OP == SMR_OP_MOD) {
            if (b == 0 || b == -1) return 0;  // (b = 0 is refused by the planner; rem(typemin, -1) = 0 without overflow)
            const ix64 r = a % b;
            if constexpr (OP == SMR_OP_MOD) return (r != 0 && ((r < 0) != (b < 0))) ? r + b : r;
            else return r;
        }
        else if constexpr (OP == SMR_OP_AND) return a & b;
        else if constexpr (OP == SMR_OP_OR) return a | b;
        else if constexpr (OP == SMR_OP_XOR) return a ^ b;
        else return a;
    }
};

template <class R>
struct mathx_cx {
    typedef cplx<R> T;
    typedef cxlim<R> L;
    // The complex functions follow Base/complex.jl where the textbook formulas lose a result that is representable: operands at the
    // ends of the range are scaled by a power of four (mid_scale), |re| beyond the point where tanh is 1 takes its own branch, and on
    // the real axis (imaginary part +-0) the real function is called and the zero keeps its sign, so that Inf * 0 never forms.
    static SMR_DEV T csqrt(T a) {
        const R s = mid_scale(a.re, a.im);             // sqrt(z) = sqrt(z * s) / sqrt(s), s a power of four
        const R x = a.re * s, y = a.im * s;
        const R back = s == R(1) ? R(1) : (s < R(1) ? R(2) : L::up_sqrt_inv);
        R r = hypot(x, y);
        if (r == R(0)) return T{R(0), a.im};
        R t = sqrt((r + fabs(x)) * R(0.5));
        const R u = (fabs(y) / (t + t)) * back;
        t *= back;
        if (x >= R(0)) return T{t, copysign(u, y)};
        return T{u, copysign(t, y)};
    }
    static SMR_DEV T clog(T a) {
        const R ax = fabs(a.re), ay = fabs(a.im);
        const R be = fmax(ax, ay), th = fmin(ax, ay);
        R re;
        if (be * be > R(0.5) && (be <= R(1.25) || be * be + th * th < R(3))) {
            // near the unit circle log|z| is small: log1p of |z|^2 - 1, formed without cancellation in its leading part
            re = log1p((be - R(1)) * (be + R(1)) + th * th) * R(0.5);
        } else {
            const R s = mid_scale(a.re, a.im);
            re = log(hypot(a.re * s, a.im * s));
            if (s != R(1)) re += (s < R(1) ? R(2) : -L::up_log2) * R(0.69314718055994530942);
        }
        return T{re, atan2(a.im, a.re)};
    }
    static SMR_DEV T un(int op, T a) {
        switch (op) {
            case SMR_OP_NEG: return -a;
            case SMR_OP_ABS: return T{hypot(a.re, a.im), R(0)};
            case SMR_OP_ABS2: return T{a.re * a.re + a.im * a.im, R(0)};
            case SMR_OP_CONJ: return T{a.re, -a.im};
            case SMR_OP_REAL: return T{a.re, R(0)};
            case SMR_OP_IMAG: return T{a.im, R(0)};
            case SMR_OP_SQRT: return csqrt(a);
            case SMR_OP_EXP: {
                R e = exp(a.re);
                if (a.im == R(0)) return T{e, a.im};
                return T{e * cos(a.im), e * sin(a.im)};
            }
            case SMR_OP_LOG: return clog(a);
            case SMR_OP_SIN:  // re = +-0: sin(iy) = i sinh(y), and 0 * cosh(y) must not meet an infinite cosh
                if (a.re == R(0)) return T{a.re, sinh(a.im)};
                return T{sin(a.re) * cosh(a.im), cos(a.re) * sinh(a.im)};
            case SMR_OP_COS:
                if (a.re == R(0)) return T{cosh(a.im), __builtin_signbit(a.im) ? a.re : -a.re};
                return T{cos(a.re) * cosh(a.im), -sin(a.re) * sinh(a.im)};
            case SMR_OP_TANH: {
                if (a.im == R(0)) return T{tanh(a.re), a.im};
                if (fabs(a.re) > L::tanh_one)  // cosh(2x) would overflow long after the quotient has become 1
                    return T{copysign(R(1), a.re), copysign(R(0), a.im * sin(fabs(a.im) + fabs(a.im)))};
                // Base's form: with t = tan(y), b = sec(y)^2, s = sinh(x), c = cosh(x): tanh(z) = (b c s + i t) / (1 + b s^2)
                const R t = tan(a.im), b = R(1) + t * t, s = sinh(a.re), c = sqrt(R(1) + s * s);
                if (t - t != R(0)) return T{c / s, R(1) / t};  // tan overflowed
                const R den = R(1) + b * s * s;
                return T{b * c * s / den, t / den};
            }
            case SMR_OP_INV: return T{R(1), R(0)} / a;
            case SMR_OP_ROUND32: return T{(R)(float)a.re, (R)(float)a.im};
        }
        return a;
    }
    static SMR_DEV T bin(int op, T a, T b) {
        switch (op) {
            case SMR_OP_ADD: return a + b;
            case SMR_OP_SUB: return a - b;
            case SMR_OP_MUL: return a * b;
            case SMR_OP_DIV: return a / b;
            case SMR_OP_MIN: return (b.re < a.re) ? b : a;
            case SMR_OP_MAX: return (a.re < b.re) ? b : a;
            case SMR_OP_LT: return T{a.re < b.re ? R(1) : R(0), R(0)};
            case SMR_OP_LE: return T{a.re <= b.re ? R(1) : R(0), R(0)};
            case SMR_OP_GT: return T{a.re > b.re ? R(1) : R(0), R(0)};
            case SMR_OP_GE: return T{a.re >= b.re ? R(1) : R(0), R(0)};
            case SMR_OP_EQ: return T{(a.re == b.re && a.im == b.im) ? R(1) : R(0), R(0)};
            case SMR_OP_NE: return T{(a.re != b.re || a.im != b.im) ? R(1) : R(0), R(0)};
        }
        return a;
    }
    static SMR_DEV bool truthy(T a) { return a.re != R(0); }

    // math opcodes (runtime-compiled kernels only).  Complex forms of x ^ n, fma, sinh, cosh, exp2, log2, log10, sign and round;
    // every other math opcode acts on the real parts and returns imaginary part 0 (front ends never send it a complex value)
    template <int N>
    static SMR_DEV T powi(T a) {
        if constexpr (N == 0) return T{R(1), R(0)};
        else if constexpr (N == 1) return a;
        else if constexpr (N == 2) return a * a;
        else if constexpr (N == 3) return a * a * a;
        else if constexpr (N == -1) return T{R(1), R(0)} / a;
        else if constexpr (N == -2) { const T i = T{R(1), R(0)} / a; return i * i; }
        else {  // Base.power_by_squaring (of inv(z) for n < 0, complex.jl)
            T x = N < 0 ? T{R(1), R(0)} / a : a;
            int p = N < 0 ? -N : N;
            int t = __builtin_ctz(p) + 1;
            p >>= t;
            while (--t > 0) x = x * x;
            T y = x;
            while (p > 0) {
                t = __builtin_ctz(p) + 1;
                p >>= t;
                while (--t >= 0) x = x * x;
                y = y * x;
            }
            return y;
        }
    }
    // Julia's muladd(::Complex, ::Complex, ::Complex) (complex.jl), every part fused
    static SMR_DEV T fma3(T a, T b, T c) {
        return T{fma(a.re, b.re, -fma(a.im, b.im, -c.re)), fma(a.re, b.im, fma(a.im, b.re, c.im))};
    }
    template <int OP>
    static SMR_DEV T ext_un(T a) {
        if constexpr (OP == SMR_OP_SINH) {  // im = +-0: the real function, and an infinite cosh must not meet the zero
            if (a.im == R(0)) return T{sinh(a.re), a.im};
            return T{sinh(a.re) * cos(a.im), cosh(a.re) * sin(a.im)};
        }
        else if constexpr (OP == SMR_OP_COSH) {
            if (a.im == R(0)) return T{cosh(a.re), __builtin_signbit(a.re) ? -a.im : a.im};
            return T{cosh(a.re) * cos(a.im), sinh(a.re) * sin(a.im)};
        }
        else if constexpr (OP == SMR_OP_EXP2) {
            const R e = exp2(a.re), th = a.im * R(0.69314718055994530942);
            if (a.im == R(0)) return T{e, a.im};
            return T{e * cos(th), e * sin(th)};
        }
        else if constexpr (OP == SMR_OP_LOG2 || OP == SMR_OP_LOG10) {  // log(z) / log(oftype(real(z), 2 or 10))
            const R d = OP == SMR_OP_LOG2 ? R(0.69314718055994530942) : R(2.30258509299404568402);
            const T l = clog(a);
            return T{l.re / d, l.im / d};
        }
        else if constexpr (OP == SMR_OP_SIGN) {
            if (a.re == R(0) && a.im == R(0)) return a;
            const R s = mid_scale(a.re, a.im);  // z / |z| of the scaled value: hypot neither overflows nor rounds among the subnormals
            const R x = a.re * s, y = a.im * s, r = hypot(x, y);
            return T{x / r, y / r};
        }
        else if constexpr (OP == SMR_OP_ROUND) return T{rint(a.re), rint(a.im)};
        else return T{mathx_real<R>::template ext_un<OP>(a.re), R(0)};
    }
    template <int OP>
    static SMR_DEV T ext_bin(T a, T b) { return T{mathx_real<R>::template ext_bin<OP>(a.re, b.re), R(0)}; }
};
template <> struct mathx<c32> : mathx_cx<float> {};
template <> struct mathx<c64> : mathx_cx<double> {};

// ---- loads / stores ------------------------------------------------------------------------
// Typed fast path: the operand's dtype is the compute type.
template <class T>
SMR_DEV T ld(const void* base, i64 idx) {
    return ((const T*)base)[idx];
}
template <class T>
SMR_DEV void st(void* base, i64 idx, T v) {
    ((T*)base)[idx] = v;
}
// Mixed path: convert from/to the operand's own dtype (wave-uniform switch).
template <class T>
SMR_DEV T ld_as(const void* base, i64 idx, int dt) {
    typedef typename tr<T>::real R;
    if constexpr (is_int_class<T>::value) {  // sign / zero extension; floating operands never reach this class
        switch (dt) {
            case SMR_I8: return ((const int8_t*)base)[idx];
            case SMR_U8: return ((const uint8_t*)base)[idx];
            case SMR_I16: return ((const int16_t*)base)[idx];
            case SMR_U16: return ((const uint16_t*)base)[idx];
            case SMR_I32: return ((const int32_t*)base)[idx];
            case SMR_U32: return ((const uint32_t*)base)[idx];
            case SMR_I64: return ((const long long*)base)[idx];
            case SMR_U64: return (ix64)((const unsigned long long*)base)[idx];
        }
        return 0;
    } else
    switch (dt) {
        case SMR_F32: return mk<T>(R(((const float*)base)[idx]), R(0));
        case SMR_F64: return mk<T>(R(((const double*)base)[idx]), R(0));
        case SMR_C32: { c32 v = ((const c32*)base)[idx]; return mk<T>(R(v.re), R(v.im)); }
        case SMR_C64: { c64 v = ((const c64*)base)[idx]; return mk<T>(R(v.re), R(v.im)); }
        case SMR_I8: return mk<T>(R(((const int8_t*)base)[idx]), R(0));
        case SMR_U8: return mk<T>(R(((const uint8_t*)base)[idx]), R(0));
        case SMR_I16: return mk<T>(R(((const int16_t*)base)[idx]), R(0));
        case SMR_U16: return mk<T>(R(((const uint16_t*)base)[idx]), R(0));
        case SMR_I32: return mk<T>(R(((const int32_t*)base)[idx]), R(0));
        case SMR_U32: return mk<T>(R(((const uint32_t*)base)[idx]), R(0));
        case SMR_I64: return mk<T>(R(((const long long*)base)[idx]), R(0));
        case SMR_U64: return mk<T>(R(((const unsigned long long*)base)[idx]), R(0));
    }
    return mk<T>(R(0), R(0));
}
template <class T>
SMR_DEV void st_as(void* base, i64 idx, int dt, T v) {
    if constexpr (is_int_class<T>::value) {  // truncation = the wrapped value in the narrower type
        switch (dt) {
            case SMR_I8: case SMR_U8: ((uint8_t*)base)[idx] = (uint8_t)v; break;
            case SMR_I16: case SMR_U16: ((uint16_t*)base)[idx] = (uint16_t)v; break;
            case SMR_I32: case SMR_U32: ((uint32_t*)base)[idx] = (uint32_t)v; break;
            case SMR_I64: case SMR_U64: ((long long*)base)[idx] = v; break;
        }
        return;
    } else {
    auto re = re_(v);
    auto im = im_(v);
    switch (dt) {
        case SMR_F32: ((float*)base)[idx] = (float)re; break;
        case SMR_F64: ((double*)base)[idx] = (double)re; break;
        case SMR_C32: ((c32*)base)[idx] = c32{(float)re, (float)im}; break;
        case SMR_C64: ((c64*)base)[idx] = c64{(double)re, (double)im}; break;
        case SMR_I8: ((int8_t*)base)[idx] = (int8_t)llrint((double)re); break;
        case SMR_U8: ((uint8_t*)base)[idx] = (uint8_t)llrint((double)re); break;
        case SMR_I16: ((int16_t*)base)[idx] = (int16_t)llrint((double)re); break;
        case SMR_U16: ((uint16_t*)base)[idx] = (uint16_t)llrint((double)re); break;
        case SMR_I32: ((int32_t*)base)[idx] = (int32_t)llrint((double)re); break;
        case SMR_U32: ((uint32_t*)base)[idx] = (uint32_t)llrint((double)re); break;
        case SMR_I64: ((long long*)base)[idx] = (long long)llrint((double)re); break;
        case SMR_U64: {
            // llrint saturates at 2^63: values of the upper half are shifted into range first
            const double d = (double)re;
            ((unsigned long long*)base)[idx] = d >= 9223372036854775808.0 ? (unsigned long long)llrint(d - 9223372036854775808.0) + 9223372036854775808ull
                                                                          : (unsigned long long)llrint(d);
            break;
        }
    }
    }
}

// Operand table passed to every kernel by value.
struct OpTab {
    void* base[MAXM];   // base pointer with the element offset already applied
    int32_t dtype[MAXM];
    int32_t conj[MAXM];
};

template <class T, bool MIXED>
SMR_DEV T load_op(const OpTab& t, int k, i64 idx) {
    T v;
    if constexpr (MIXED)
        v = ld_as<T>(t.base[k], idx, t.dtype[k]);
    else
        v = ld<T>(t.base[k], idx);
    if constexpr (tr<T>::cx) {
        if (t.conj[k]) v = cj(v);
    }
    return v;
}
template <class T, bool MIXED>
SMR_DEV void store_op(const OpTab& t, i64 idx, T v) {
    if constexpr (tr<T>::cx) {
        if (t.conj[0]) v = cj(v);
    }
    if constexpr (MIXED)
        st_as<T>(t.base[0], idx, t.dtype[0], v);
    else
        st<T>(t.base[0], idx, v);
}

// ---- functors: f(a[0..NIN-1]) ---------------------------------------------------------------
// NIN < 0 means "runtime" (interpreter).  Constants come from Canon::fc.
// A functor with constants also takes them on the device: set_consts(k) rebuilds them from a row of doubles laid out like
// Canon::fc (a program: like ProgD::consts), converted as hostmk<T> converts on the host.  A grouped launch whose members have
// scalars of their own (smr_k_group.hip) calls it with the member's row; P is a pointer to double in any address space.
template <class T, class P> SMR_DEV T mk_const(P k, int i) {
    typedef typename tr<T>::real R;
    return mk<T>(rcast<R>(k[2 * i]), rcast<R>(k[2 * i + 1]));
}
template <class T> struct FIdent {
    static constexpr int NIN = 1;
    SMR_DEV T operator()(const T* a) const { return a[0]; }
};
template <class T> struct FAdd2 {
    static constexpr int NIN = 2;
    SMR_DEV T operator()(const T* a) const { return a[0] + a[1]; }
};
template <class T> struct FAdd3 {
    static constexpr int NIN = 3;
    SMR_DEV T operator()(const T* a) const { return (a[0] + a[1]) + a[2]; }
};
template <class T> struct FAdd4 {
    static constexpr int NIN = 4;
    SMR_DEV T operator()(const T* a) const { return ((a[0] + a[1]) + a[2]) + a[3]; }
};
template <class T> struct FScale {
    static constexpr int NIN = 1;
    T c;
    template <class P> SMR_DEV void set_consts(P k) { c = mk_const<T>(k, 0); }
    SMR_DEV T operator()(const T* a) const { return a[0] * c; }
};
template <class T> struct FSym {
    static constexpr int NIN = 2;
    T c;
    template <class P> SMR_DEV void set_consts(P k) { c = mk_const<T>(k, 0); }
    SMR_DEV T operator()(const T* a) const {
        // complex: the plain Smith quotient (no scaling at the ends of the range: the divisor is the call's constant, and the scaled
        // form costs the pipelined ComplexF64 TILED kernel of this functor 12 bytes of scratch, which a recorded sequence cannot take)
        if constexpr (tr<T>::cx) return div_smith(a[0] + a[1], c);
        else return mathx<T>::bin(SMR_OP_DIV, a[0] + a[1], c);
    }
};
template <class T> struct FAxpy {
    static constexpr int NIN = 2;
    T c;
    template <class P> SMR_DEV void set_consts(P k) { c = mk_const<T>(k, 0); }
    SMR_DEV T operator()(const T* a) const { return c * a[0] + a[1]; }
};
template <class T> struct FAxpby {
    static constexpr int NIN = 2;
    T c, d;
    template <class P> SMR_DEV void set_consts(P k) { c = mk_const<T>(k, 0); d = mk_const<T>(k, 1); }
    SMR_DEV T operator()(const T* a) const { return c * a[0] + d * a[1]; }
};
template <class T> struct FAbs2 {
    static constexpr int NIN = 1;
    SMR_DEV T operator()(const T* a) const { return mathx<T>::un(SMR_OP_ABS2, a[0]); }
};
template <class T> struct FMul2 {
    static constexpr int NIN = 2;
    SMR_DEV T operator()(const T* a) const { return a[0] * a[1]; }
};
// the mul! form x * y * alpha of a contraction group with an alpha per member (smr_k_gcontract.hip): the program `arg1 arg2 MUL const
// MUL` with the program's own multiply (complex, wrapping Int64), so that it is bit-equal to the program run as a program
template <class T> struct FMul2Scale {
    static constexpr int NIN = 2;
    T c;
    template <class P> SMR_DEV void set_consts(P k) { c = mk_const<T>(k, 0); }
    SMR_DEV T operator()(const T* a) const { return mathx<T>::bin(SMR_OP_MUL, mathx<T>::bin(SMR_OP_MUL, a[0], a[1]), c); }
};
template <class T> struct FExpr5 {  // a*exp(c*a) + sin(a*a), real types only
    static constexpr int NIN = 1;
    T c;
    template <class P> SMR_DEV void set_consts(P k) { c = mk_const<T>(k, 0); }
    SMR_DEV T operator()(const T* a) const {
        T x = a[0];
        if constexpr (is_int_class<T>::value) return x;  // never selected for the integer class
        else return x * exp(c * x) + sin(x * x);
    }
};

// Bytecode interpreter.  The program is wave-uniform, so every branch below is a scalar
// branch; the value stack lives in registers and is rotated on push/pop so that every
// register index is static (runtime-indexed arrays would be demoted to scratch memory).
template <class T> struct FProg {
    static constexpr int NIN = -1;
    ProgD p;
    template <class P> SMR_DEV void set_consts(P k) {  // the row holds 2 * nconst doubles, no more
#pragma unroll
        for (int i = 0; i < 2 * SMR_MAXCONST; ++i)
            if (i < 2 * p.nconst) p.consts[i] = k[i];
    }
    SMR_DEV T operator()(const T* a) const {
        typedef typename tr<T>::real R;
        T s0 = mk<T>(R(0), R(0)), s1 = s0, s2 = s0, s3 = s0, s4 = s0, s5 = s0, s6 = s0, s7 = s0;
        const int n = p.len;
        for (int pc = 0; pc < n; ++pc) {
            const int op = p.code[2 * pc], imm = p.code[2 * pc + 1];
            if (op <= SMR_OP_CONST) {
                T v;
                if (op == SMR_OP_ARG) {
                    v = a[0];
#pragma unroll
                    for (int k = 1; k < MAXIN; ++k)
                        if (imm == k + 1) v = a[k];
                } else {
                    v = mk<T>(rcast<R>(p.consts[2 * imm]), rcast<R>(p.consts[2 * imm + 1]));
                }
                s7 = s6; s6 = s5; s5 = s4; s4 = s3; s3 = s2; s2 = s1; s1 = s0; s0 = v;
            } else if (op < 32) {
                s0 = mathx<T>::un(op, s0);
            } else if (op < 64) {
                s0 = mathx<T>::bin(op, s1, s0);
                s1 = s2; s2 = s3; s3 = s4; s4 = s5; s5 = s6; s6 = s7;
            } else {  // SELECT: a ? b : c with a=s2, b=s1, c=s0
                s0 = mathx<T>::truthy(s2) ? s1 : s0;
                s1 = s3; s2 = s4; s3 = s5; s4 = s6; s5 = s7;
            }
        }
        return s0;
    }
};

// reduction operator / initop (wave-uniform switches)
template <class T>
SMR_DEV T red_apply(int op, T a, T b) {
    if constexpr (tr<T>::arith) {
        switch (op) {
            case SMR_RED_ADD: return a + b;
            case SMR_RED_MUL: return a * b;
            case SMR_RED_MIN: return mathx<T>::bin(SMR_OP_MIN, a, b);
            case SMR_RED_MAX: return mathx<T>::bin(SMR_OP_MAX, a, b);
            case SMR_RED_AND: return mk<T>((mathx<T>::truthy(a) && mathx<T>::truthy(b)) ? typename tr<T>::real(1) : typename tr<T>::real(0), typename tr<T>::real(0));
            case SMR_RED_OR: return mk<T>((mathx<T>::truthy(a) || mathx<T>::truthy(b)) ? typename tr<T>::real(1) : typename tr<T>::real(0), typename tr<T>::real(0));
        }
    }
    return b;
}
// the neutral element of a reduction operator: the seed of every accumulator (smr_k_reduce.hip, smr_k_contract.hip)
template <class T>
SMR_DEV T neutral(int op) {
    typedef typename tr<T>::real R;
    switch (op) {
        case SMR_RED_MUL: return mk<T>(R(1), R(0));
        case SMR_RED_AND: return mk<T>(R(1), R(0));
        case SMR_RED_MIN: return mk<T>(rcast<R>(__builtin_huge_val()), R(0));   // integer class: typemax / typemin
        case SMR_RED_MAX: return mk<T>(rcast<R>(-__builtin_huge_val()), R(0));
        case SMR_RED_ADD:
            // the identity of IEEE addition is -0.0: x + (-0.0) == x bit for bit for every x, +0.0 included, while (-0.0) + (+0.0) is
            // +0.0 -- accumulators and the partials of empty chunks seeded with +0.0 turned a sum of -0.0 into +0.0
            // The zero is made opaque in a vector register and negated there.  Written as the constant (-0.0, -0.0), the seed of the folds
            // that take `op` at run time (k_reduce_final, k_reduce_part_final) sits in scalar registers, and for ComplexF64 the compiler's
            // assembly sets the imaginary part by `s_mov_b64 s[2:3], 0x8000000000000000`.  gfx950 has no 64-bit scalar literal: the
            // object holds the instruction with the low 32 bits only (disassembled: `s_mov_b64 s[2:3], 0`), +0.0.
            if constexpr (!is_int_class<T>::value) {
                R z = R(0);
                asm volatile("" : "+v"(z));
                return mk<T>(-z, -z);
            }
            break;
    }
    return mk<T>(R(0), R(0));
}

template <class T>
SMR_DEV T init_apply(int op, T x, T beta) {
    typedef typename tr<T>::real R;
    switch (op) {
        case SMR_INIT_ZERO: return mk<T>(R(0), R(0));
        case SMR_INIT_SCALE: return x * beta;
        case SMR_INIT_CONST: return beta;
        case SMR_INIT_CONJ: return cj(x);
    }
    return x;
}

// wave64 shuffle of arbitrary POD (by 32-bit words)
template <class T>
SMR_DEV T shfl_xor_any(T v, int mask) {
    static_assert(sizeof(T) % 4 == 0, "word multiple");
    union {
        T t;
        int w[sizeof(T) / 4];
    } u;
    u.t = v;
#pragma unroll
    for (int i = 0; i < (int)(sizeof(T) / 4); ++i) u.w[i] = __shfl_xor(u.w[i], mask, 64);
    return u.t;
}

}  // namespace smr
