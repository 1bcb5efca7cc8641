/*
 * strided_hip.h -- C ABI of libstrided_hip.so: the MI355X (gfx950) implementation of
 * Strided.jl's fused N-ary strided map / map-reduce engine.
 *
 * Drop-in boundary.  The reference has no FFI; its single internal
 * funnel is
 *     _mapreduce_fuse!(f, op, initop, dims::Dims, arrays::Tuple{Vararg{StridedView}})
 *                                                   (reference src/mapreduce.jl:98-117)
 * reached from map! (src/mapreduce.jl:50), broadcast copyto! (src/broadcast.jl:35) and
 * _mapreducedim! (src/mapreduce.jl:93).  A Julia method specialised on a device-backed
 * parent array serialises its arguments into an `smr_problem` and `ccall`s `smr_mapreduce`
 * (binding shown in INTEGRATION.md / julia/StridedHIP.jl).  Plain C: pointers, sizes and
 * PODs only, no exceptions, no C++ or torch types.
 *
 * Conventions
 *  - Column-major, strides and offsets in ELEMENTS, 0-based:
 *        element (i_1..i_N), 0 <= i_k < dims[k], of operand j lives at
 *        ((T*)ops[j].base)[ ops[j].offset + sum_k i_k * ops[j].strides[k] ]
 *    (the reference's 1-based ParentIndex = offset + 1 + sum (i_k-1)*stride_k,
 *     src/mapreduce.jl:268).  Strides may be 0 (broadcast / reduced dim,
 *    src/broadcast.jl:50-65) or negative (reversed ranges).
 *  - ops[0] is the destination (arrays[1] of the reference), ops[1..M-1] are the inputs.
 *  - redop == SMR_RED_NONE : pure map, destination overwritten with f(inputs...)
 *    (kernel body src/mapreduce.jl:310-312).
 *    redop != NONE : dest[I] = op(dest[I], f(inputs...)) accumulated over every index that
 *    maps to the same destination element (dims with destination stride 0),
 *    src/mapreduce.jl:313-316.  The existing destination content takes part, after
 *    `initop` (if any) was applied to it exactly once (src/mapreduce.jl:351-382,403-409).
 *  - `conj` on an input: the loaded value is conjugated; on the destination: loads and
 *    stores conjugate (StridedView.op in {identity, conj}, ParentIndex get/set,
 *    src/mapreduce.jl:276-278, src/linalg.jl:50).
 *  - No dimension may be 0 (callers return early: src/mapreduce.jl:48,88-91).
 *  - All entry points return 0 (SMR_OK) or a negative smr_status; a human-readable
 *    message for the calling thread's last failure is available from smr_last_error().
 *    The reference throws DimensionMismatch etc. on the Julia side before the funnel
 *    (src/mapreduce.jl:43-46, src/broadcast.jl:61); the engine itself never throws.
 *  - Device pointers must belong to the current HIP device of the calling thread.
 *    Calls are asynchronous on `stream` (NULL = the null stream); the caller keeps the
 *    buffers alive until the stream reaches the kernels.
 */
#ifndef STRIDED_HIP_H
#define STRIDED_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMR_ABI_VERSION 1
#define SMR_MAXN 8      /* max rank of the iteration box (reference tests go to N = 6)   */
#define SMR_MAXM 8      /* max operands including the destination                        */
#define SMR_MAXPROG 96  /* max instructions in an f-program                              */
#define SMR_MAXCONST 16 /* max (complex) constants captured by an f-program              */

typedef enum {
    SMR_OK = 0,
    SMR_EINVAL = -1,       /* malformed problem (rank, dims, program, null pointers)      */
    SMR_EUNSUPPORTED = -2, /* valid in the reference but outside the device whitelist ->
                              the host shim falls back to the CPU method                  */
    SMR_EHIP = -3,         /* a HIP runtime call failed                                   */
    SMR_ENOMEM = -4,
    SMR_ENODEVICE = -5     /* no usable gfx950 device                                     */
} smr_status;

/* Element types.  Arithmetic is done in one of the four float classes every reference
 * test-set iterates over (test/othertests.jl:2), or -- round 3 -- in the INTEGER class: when every
 * operand (destination included) has an integer eltype and f uses only integer-closed operations
 * (+ - * neg abs abs2 min max comparisons select, integer-valued constants; reductions + * min max & |),
 * the call computes in wrapping 64-bit two's-complement arithmetic like Julia's Int64 (sum of an Int64
 * view above 2^53, overflow wrap-around) and truncates on store to a narrower destination type (= the
 * wrapped result of Julia's arithmetic in that type for + - * chains); where Julia would observe a narrow
 * intermediate result at its own width (an order / equality test on it, a conversion to a wider type, a wider
 * destination) the library re-wraps the 64-bit value to that type (SMR_OP_WRAP_*, inserted by the planner),
 * so Int32 a .* b into an Int64 array is the wrapped 32-bit product.  UInt64 operands take part in ring
 * operations only (no order: min / max / < / abs are refused with SMR_EUNSUPPORTED, as is any 64-bit integer
 * input that meets floating-point arithmetic).  Pure moves (copy!/permutedims!) of any integer width are
 * bit copies; integers mixed with floats compute in Float64.                                             */
typedef enum {
    SMR_F32 = 0,
    SMR_F64 = 1,
    SMR_C32 = 2, /* ComplexF32: interleaved (re, im) float  */
    SMR_C64 = 3, /* ComplexF64: interleaved (re, im) double */
    SMR_I8 = 4,
    SMR_I16 = 5,
    SMR_I32 = 6,
    SMR_I64 = 7,
    SMR_U8 = 8,
    SMR_U16 = 9,
    SMR_U32 = 10,
    SMR_U64 = 11,
    SMR_BOOL = 12, /* Julia's Bool / NumPy's bool_: one byte holding 0 or 1.  Moves and computes like a UInt8; what differs is Julia's
                      typing of f (Bool yields to every integer type: true + Int8(1) is an Int8, -true and true + true are Ints) */
    SMR_DTYPE_COUNT = 13
} smr_dtype;

/* Reduction operator `op` (neutral elements follow _init_reduction!,
 * src/mapreduce.jl:182-191; the caller pre-fills the destination).                      */
typedef enum {
    SMR_RED_NONE = 0,
    SMR_RED_ADD = 1, /* +, Base.add_sum */
    SMR_RED_MUL = 2, /* *, Base.mul_prod */
    SMR_RED_MIN = 3,
    SMR_RED_MAX = 4,
    SMR_RED_AND = 5, /* &: both operands non-zero -> 1, else 0 (neutral element true, :188)  */
    SMR_RED_OR = 6   /* |  (neutral element false, :189)                                     */
} smr_redop;

/* `initop`, applied once to each destination element before accumulation.  These are
 * exactly the five forms the reference exercises (test/othertests.jl:76-102,
 * src/linalg.jl:146-160).                                                               */
typedef enum {
    SMR_INIT_NONE = 0,     /* nothing            */
    SMR_INIT_IDENTITY = 1, /* identity           */
    SMR_INIT_ZERO = 2,     /* zero / x -> 0      */
    SMR_INIT_SCALE = 3,    /* x -> x * beta      (beta = initarg[0] + i*initarg[1])      */
    SMR_INIT_CONST = 4,    /* x -> beta                                                   */
    SMR_INIT_CONJ = 5      /* conj                                                        */
} smr_initop;

/* f-program: the fused N-ary elementwise function f (the CaptureArgs functor tree of
 * src/broadcast.jl:67-98, or map!'s closure) serialised as postfix code, two bytes per
 * instruction: {opcode, immediate}.  The program must leave exactly one value.
 * Opcode ranges: 0..7 push, unary 8..31 and 96..127, binary 32..63 and 128..159, ternary 64..95.
 * The opcodes from 65 and from 96 on (the "math" opcodes: powers, fma, more of Base's math and the bitwise
 * operations) run in runtime-compiled kernels only: a plan that would interpret such a program (option
 * "jit" = 0, or no runtime compiler) is refused with SMR_EUNSUPPORTED.  Where Julia throws (DomainError),
 * they give the IEEE result (pow(-8.0, 1/3) is NaN).                                      */
typedef enum {
    SMR_OP_ARG = 0,   /* push input #imm (1-based: ops[imm]), conj flag applied           */
    SMR_OP_CONST = 1, /* push fconsts[2*imm] + i*fconsts[2*imm+1]                         */
    /* unary: pop 1, push 1 */
    SMR_OP_NEG = 8,
    SMR_OP_ABS = 9,
    SMR_OP_ABS2 = 10,
    SMR_OP_CONJ = 11,
    SMR_OP_REAL = 12,
    SMR_OP_IMAG = 13,
    SMR_OP_SQRT = 14,
    SMR_OP_EXP = 15,
    SMR_OP_LOG = 16,
    SMR_OP_SIN = 17,
    SMR_OP_COS = 18,
    SMR_OP_TANH = 19,
    SMR_OP_INV = 20,
    SMR_OP_ROUND32 = 21, /* round to Float32 (each part of a complex value): the host inserts it after
                            every operation Julia would have carried out in Float32 / ComplexF32 while
                            the call as a whole computes in Float64 (per-operation typing)         */
    SMR_OP_WIDEN = 22,   /* identity; its presence makes the call compute in the 64-bit class although no
                            operand is 64-bit: a Float64 / ComplexF64 scalar meets Float32 arrays
                            (`B32 .= A32 .* 0.1` multiplies in Float64 in Julia and rounds once on store) */
    /* 23..28 are the library's own: a user program holding one is malformed (SMR_EINVAL).  The integer class inserts them where
       Julia would have observed a narrow intermediate result at its own width (Int32 a .* b into an Int64 destination, UInt8
       min(a - b, c), ...): the 64-bit value is reduced to its low 8 / 16 / 32 bits, sign- or zero-extended (csrc/smr_canon.cpp) */
    SMR_OP_WRAP_I8 = 23,
    SMR_OP_WRAP_I16 = 24,
    SMR_OP_WRAP_I32 = 25,
    SMR_OP_WRAP_U8 = 26,
    SMR_OP_WRAP_U16 = 27,
    SMR_OP_WRAP_U32 = 28,
    /* binary: pop b, pop a, push a (op) b */
    SMR_OP_ADD = 32,
    SMR_OP_SUB = 33,
    SMR_OP_MUL = 34,
    SMR_OP_DIV = 35,
    SMR_OP_MIN = 36,
    SMR_OP_MAX = 37,
    SMR_OP_LT = 38, /* comparisons act on real parts and push 1.0 / 0.0                   */
    SMR_OP_LE = 39,
    SMR_OP_GT = 40,
    SMR_OP_GE = 41,
    SMR_OP_EQ = 42,
    SMR_OP_NE = 43,
    /* ternary: pop c, pop b, pop a, push (real(a) != 0 ? b : c)                           */
    SMR_OP_SELECT = 64,
    SMR_OP_FMA = 65, /* fma(a, b, c) and muladd(a, b, c): fused on real types; complex: Julia's muladd(::Complex, ...) with fused parts */
    /* unary math (runtime-compiled kernels only) */
    SMR_OP_POWI = 96, /* Base.literal_pow(^, x, Val(n)) / x ^ n for an integer literal n = imm as int8 (-128..127): n = 0 1 2 3 -1 -2
                         are one(x), x, x*x, x*x*x, inv(x), inv(x)^2; other n: Float32 via Float64 pown rounded once, Float64
                         pown, complex power_by_squaring (of inv(x) for n < 0), integers (n >= 0 only) wrapping        */
    SMR_OP_TAN = 97,
    SMR_OP_ASIN = 98,
    SMR_OP_ACOS = 99,
    SMR_OP_ATAN = 100,
    SMR_OP_SINH = 101,
    SMR_OP_COSH = 102,
    SMR_OP_EXP2 = 103,
    SMR_OP_EXPM1 = 104,
    SMR_OP_LOG2 = 105,
    SMR_OP_LOG10 = 106,
    SMR_OP_LOG1P = 107,
    SMR_OP_CBRT = 108,
    SMR_OP_FLOOR = 109,
    SMR_OP_CEIL = 110,
    SMR_OP_TRUNC = 111,
    SMR_OP_ROUND = 112, /* RoundNearest: ties to even (each part of a complex value)                                    */
    SMR_OP_SIGN = 113,  /* keeps NaN and +-0; complex: z / abs(z), 0 for z = 0                                          */
    SMR_OP_NOT = 114,   /* ~ on integers (bitwise complement); Bool ! / ~ is XOR with true                              */
    /* binary math (runtime-compiled kernels only); ops without a complex form act on real parts (imaginary part 0) */
    SMR_OP_POW = 128,   /* a ^ b                                                                                        */
    SMR_OP_ATAN2 = 129, /* atan(a, b) = atan(y, x)                                                                      */
    SMR_OP_HYPOT = 130,
    SMR_OP_REM = 131,   /* rem (Julia's %): truncated, the sign of a; integers: non-zero constant divisors only          */
    SMR_OP_MOD = 132,   /* mod: floored, the sign of b; integers: non-zero constant divisors only                       */
    SMR_OP_AND = 133,   /* & | xor on integer (and Bool) values; in a float class on the values converted to Int64       */
    SMR_OP_OR = 134,
    SMR_OP_XOR = 135
} smr_opcode;

/* One StridedView operand: (parent, size, strides, offset, op) of the reference's
 * StridedView (5-argument constructor call src/broadcast.jl:64) minus the shared size.  */
typedef struct smr_operand {
    void* base;                /* device pointer to parent[0]                             */
    int64_t offset;            /* element offset of the view's first element              */
    int64_t strides[SMR_MAXN]; /* element strides; 0 = broadcast/reduced; may be < 0      */
    int32_t dtype;             /* smr_dtype                                               */
    int32_t conj;              /* 0 = identity, 1 = conj                                  */
} smr_operand;

/* The fully lowered argument list of _mapreduce_fuse! (src/mapreduce.jl:98-99). */
typedef struct smr_problem {
    int32_t N;              /* rank of the iteration box, 1..SMR_MAXN                     */
    int32_t M;              /* operands incl. destination, 2..SMR_MAXM (1 allowed when
                               the program has no ARG, e.g. fill)                         */
    int64_t dims[SMR_MAXN]; /* common size of all operands, every entry >= 1             */
    smr_operand ops[SMR_MAXM];
    const uint8_t* fprog; /* 2*fprog_len bytes; NULL/0 = identity on ops[1]             */
    int32_t fprog_len;
    int32_t nconsts;
    const double* fconsts; /* 2*nconsts doubles (re, im)                                 */
    int32_t redop;         /* smr_redop                                                  */
    int32_t initop;        /* smr_initop, only with redop != NONE                        */
    double initarg[2];     /* beta for SCALE / CONST                                     */
    void* stream;          /* hipStream_t, NULL = null stream                            */
} smr_problem;

typedef struct smr_plan smr_plan; /* opaque: canonicalised problem + chosen kernel */

/* ---- library / device ---------------------------------------------------------------- */
int smr_abi_version(void);
/* Bind the calling thread to `device` (>= 0) and create the per-device state.  Replaces
 * the reference's thread-count configuration (src/Strided.jl:18-35,50-52).             */
int smr_init(int device);
int smr_shutdown(void);
int smr_device_count(void);
const char* smr_last_error(void);
/* Device memory for hosts without their own allocator (the Julia shim's HipBuffer).     */
int smr_malloc(size_t bytes, void** out);
int smr_free(void* p);
int smr_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int smr_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
int smr_stream_sync(void* stream);

/* ---- overlap windows: independent launches of one stream may run concurrently -----------------
 * The reference runs the independent halves of a problem as concurrent tasks and waits only where it
 * must (src/mapreduce.jl:203-223).  smr_overlap_begin(stream) / smr_overlap_end(stream) mark such a stretch of
 * work on `stream`; windows nest, and an end without a matching begin returns SMR_EINVAL.  For launches that go
 * through HIP a window is a no-op: they stay stream-ordered (HIP accepts hipExtAnyOrderLaunch and ignores it on
 * gfx9, measured with device stamps, profiles/r04_overlap.txt).  smr_overlap_fence(stream) orders everything the
 * library launched on `stream` before work the caller queues there next; on a library-owned stream it waits for
 * the library's direct launches.  Independent launches DO overlap where the library dispatches by itself: on
 * the streams of smr_stream_create (next paragraph) and in recorded sequences (smr_seq_*).
 * smr_stream_create returns a stream of the library's own -- the stream of a host (the Julia shim) that routes ALL its device work
 * through this library.  On MI355X its launches do not go through HIP at all: the library submits every launch itself as an AQL
 * packet on one of four HSA queues it owns, choosing the queue by the data -- a launch that conflicts with nothing in flight goes to
 * the least loaded queue and runs concurrently with its predecessors, one that conflicts with launches on one queue follows them
 * there, one that conflicts with several queues waits for them through a barrier-AND packet; completion signals retire the ranges
 * (csrc/smr_eager.cpp: eager direct dispatch; ~1 us of host time per launch instead of HIP's 3.6-4 us).  Results are those of in-order
 * execution.  The library fences by itself (waits for its queues) before every copy / synchronisation / sequence replay it performs on
 * such a stream (smr_memcpy_*, smr_stream_sync, smr_mapreduce_scalar, smr_seq_run, smr_free, smr_plan_destroy) and drains the HIP
 * work it queued there before the next direct launch.  Option "eager_direct" = 0 sends the launches through HIP instead, in stream
 * order.                                                                                      */
int smr_overlap_begin(void* stream);
int smr_overlap_end(void* stream);
int smr_overlap_fence(void* stream);
int smr_stream_create(void** out);
int smr_stream_destroy(void* stream);

/* ---- recorded sequences: the library's own replay of a list of plan and group executions ----------
 * smr_seq_add records executions of plans (with optional rebinding of base pointers, as smr_plan_execute);
 * smr_seq_add_group records one execution of a group (smr_group_*, below: K small maps as one launch) -- a sequence may mix
 * both kinds in any order, and a group is ONE step of the list: one packet per replay, no host call per execution.  Its footprint
 * is the union of its members' operand ranges (reads: every input; writes: every destination; kept merged by smr_group_create,
 * also under SMR_GROUP_INDEPENDENT, where they are the conservative bounding ranges).  A group's base pointers are fixed (no
 * rebinding) and the group must outlive the sequence.  Its workgroups are independent, so a component that is one group launch
 * can be cut into block ranges over several queues ("slices" below), runtime-compiled f included.
 * smr_seq_run(seq, reps, stream) performs the recorded list `reps` times with the results of in-order
 * execution on `stream`.  On MI355X the replay does not go through HIP's launch path: every launch
 * becomes a pre-built AQL dispatch packet (kernel object of the code object HIP loaded, kernarg block
 * resident in device memory) on HSA queues the library owns.  The recorded executions are split into
 * dependency components -- two executions belong together when one writes bytes the other reads or
 * writes (operand footprints and the plans' own partials) -- and every component keeps its recorded
 * order on ONE queue, while different components run on different queues (up to 4), concurrently: the
 * device form of src/mapreduce.jl:203-223 (spawn what is independent, wait where it must).  Inside one
 * queue MI355X runs consecutive dispatches one after the other whatever the barrier bit says, and a
 * kernel boundary costs 1.6-1.9 us there (profiles/r04_overlap.txt); two queues overlap one chain's
 * boundary with the other chain's kernel.  A replay costs ~0.1 us of host time per launch instead of
 * HIP's 3.6-4 us.  Work queued on `stream` before the call completes first (the call waits for it on
 * the host when the stream is busy).  smr_seq_run is ASYNCHRONOUS (round 5): it returns when the doorbells are rung -- like the
 * reference's @spawn, whose `wait` is a separate step (src/mapreduce.jl:214-223) -- and work queued on `stream` afterwards still
 * comes after the replay:
 *   - a library-owned stream (smr_stream_create): everything on it goes through this library, which waits for the replay before
 *     whatever it submits or does there next;
 *   - a HIP stream: hipStreamWaitValue64 on the completion signals where the device offers it ($SMR_SEQ_STREAM_WAIT=1), otherwise a
 *     one-wave holding kernel on the stream that polls the signals (bounded by $SMR_DIRECT_TIMEOUT_MS; smr_seq_wait reports a
 *     hold that gave up).
 * smr_seq_wait blocks the host until the last replay has completed (active wait on the signals: microseconds sooner than
 * hipStreamSynchronize).  smr_seq_set "async" = 0 makes smr_seq_run itself wait.  Runtime-compiled kernels take part like
 * precompiled ones (their entry points carry a per-program name; the sequence co-owns the loaded program).  A sequence holding a
 * kernel that needs scratch memory is replayed through HIP, in order (smr_seq_info tells which, and reports "last_replay_us":
 * first doorbell -> completion observed; "kernarg_layout": how the hidden-argument offsets of the packets are known -- "metadata"
 * = read from the code objects' NT_AMDGPU_METADATA notes, "+verified" = a self-test packet saw the blockDim / gridDim / LDS it was
 * given; csrc/smr_kmeta.cpp).
 * Failure: an HSA queue error, or a completion signal that does not arrive within $SMR_DIRECT_TIMEOUT_MS (default 30 s), marks the
 * device's direct path as failed -- the call that notices returns SMR_EHIP, nothing waits on those queues again, and later
 * executions and replays go through HIP.
 * One replay per device is in flight at a time.  The recorded base pointers / plans must stay alive
 * while the sequence exists.                                                                         */
typedef struct smr_seq smr_seq;
int smr_seq_create(smr_seq** out);
int smr_seq_add(smr_seq* seq, smr_plan* plan, void* const* bases);
struct smr_group;
int smr_seq_add_group(smr_seq* seq, struct smr_group* group);
int smr_seq_run(smr_seq* seq, int reps, void* stream);
int smr_seq_wait(smr_seq* seq);
int smr_seq_info(smr_seq* seq, char* buf, size_t buflen);
/* The dependency analysis alone (host arithmetic on strides and base pointers, no device needed): comp[i] = dependency component
 * of recorded execution i (numbered in order of first appearance); returns the number of components or a negative status.      */
int smr_seq_components(smr_seq* seq, int32_t* comp, size_t cap);
/* The fence analysis alone (host arithmetic too): acquire[i] = 1 when execution i reads bytes some execution of the sequence writes
 * (only those packets acquire inside a replay), *footprint = bytes of the union of every range the sequence touches,
 * *cache_resident = 1 when that is within option "self_release_max_total" (launches may then be self-released).  Returns the number
 * of recorded executions or a negative status.                                                                                       */
int smr_seq_fences(smr_seq* seq, int32_t* acquire, size_t cap, int64_t* footprint, int32_t* cache_resident);
/* "queues" (1..8, default 4: hardware queues a replay may spread over; 1 = everything in recorded order on one queue; more than 4
 * are time-multiplexed by the hardware scheduler); "slices" (-1 | 1..8: a component that consists of ONE launch of independent
 * workgroups is cut into that many contiguous block ranges, one queue each -- the device form of _mapreduce_threaded!'s bisection;
 * -1, the default: only the heaviest such component is cut, in two, when a third queue is free); "slices:<c>" (block ranges of
 * component c alone); "async" (-1 default / 0 blocking smr_seq_run / 1).
 * Fences of the packets inside a replay: "acquire" (-1 default: agent scope only on packets that read bytes the sequence writes --
 * an acquire invalidates the L2s, i.e. the read-only inputs of everything in flight; 0 none, 1 agent, 2 system on every packet),
 * "release" (1 agent, default; 2 system; 0 none: an EXPERIMENT, write-after-write across XCDs needs the write-back).
 * Experiments: "fence_scope" (both at once), "first_acquire" / "last_release" (scope of a replay's first / last packet, default 2),
 * "order" (0: every packet carries the barrier bit, 1: only those that conflict with an earlier one in flight) */
int smr_seq_set(smr_seq* seq, const char* name, int64_t value);
int smr_seq_destroy(smr_seq* seq);
/* Diagnostics (no device needed): the kernarg layout csrc/smr_kmeta.cpp reads from an AMDGPU code object image.  out[0..19] =
 * kernarg_size, explicit_end, nargs_explicit, hidden block_count x/y/z, group_size x/y/z, remainder x/y/z, global_offset x/y/z,
 * grid_dims, dynamic_lds_size offsets (-1 = not declared), needs_runtime, private_size, group_static.  `symbol` = "<mangled>.kd", or
 * NULL with index >= 0 to enumerate (the symbol is copied to name_out).  Returns the number of kernels, negative on a parse error. */
int smr_debug_kernarg_layout(const void* elf, size_t bytes, const char* symbol, int index, int32_t* out, char* name_out, size_t name_cap);
/* Test hook, host-only: the f-program the kernels of this problem would run -- the caller's program after canonicalisation, i.e.
   with the SMR_OP_WRAP_* instructions of the integer class in place.  code receives min(2 * length, cap) bytes (opcode, immediate
   pairs; SMR_OP_ARG immediates number the canonical operands: orig[j], SMR_MAXM entries, is the caller's index of operand j, -1 past
   the end -- unused and repeated operands are dropped); *nwraps the number of added instructions, *compute_class the SMR_* dtype
   computed in (-1: a bit copy).  Output pointers may be null.  Returns the length in instructions, or the (negative) error code. */
int smr_debug_canon_prog(const smr_problem* problem, uint8_t* code, int cap, int* nwraps, int* compute_class, int32_t* orig);
/* Test hook, host-only: the replay scheduler of recorded sequences (csrc/smr_sched.cpp) on `nexec` synthetic executions.  Per
   execution i: nspans[2i], nspans[2i+1] = how many byte ranges it reads / writes; `spans` holds them all in that order as [lo, hi)
   pairs; launches[5i..] = number of launches, grid of the first, first launch sliceable? (bit 1 set: a two-launch execution whose second launch folds the whole first one, SchedExec::fold_after), every launch self-released?, same_as (index
   of the first execution with the same plan and base pointers).  knobs = max_queues, slices, all_ordered, self_release_max_total,
   number of (component, slices) pairs in comp_slices.  Results: per_exec[4i..] = component, acquire, first queue, slices;
   totals[0..3] = components, sliced components, queues, cache_resident; *footprint = bytes of the union of all ranges;
   packets[8n..] = queue, execution, launch, slice, lo, hi, barrier, acquire of packet n, queue by queue in submission order (at most
   packet_cap rows).  Output pointers may be null.  Returns the number of packets, or the (negative) error code. */
int smr_debug_seq_schedule(int nexec, const int32_t* nspans, const int64_t* spans, const int32_t* launches, const int64_t* knobs, const int32_t* comp_slices,
                           int32_t* per_exec, int32_t* totals, int64_t* footprint, int32_t* packets, int packet_cap);


/* ---- the hot path --------------------------------------------------------------------- */
/* One-shot replacement of _mapreduce_fuse! (src/mapreduce.jl:98): canonicalise, pick the
 * kernel family, launch on problem->stream.  Plans are cached per problem signature.    */
int smr_mapreduce(const smr_problem* problem);
/* Complete reduction returning its value to the host: runs `problem` (whose destination is
 * ONE device element: every destination stride 0 or dim 1), waits for problem->stream and
 * copies the destination element (its own dtype) to host_result.  The synchronous tail of
 * `_mapreduce` (src/mapreduce.jl:70-71: `return out[ParentIndex(1)]`).                    */
int smr_mapreduce_scalar(const smr_problem* problem, void* host_result);

/* Planned form (the planner is the analogue of _mapreduce_order!/_mapreduce_block!/
 * _computeblocks, src/mapreduce.jl:119-180,452-500, evaluated once and reused).          */
int smr_plan_create(const smr_problem* problem, smr_plan** out);
/* `bases` (optional, M entries) rebinds the operand base pointers; NULL keeps the ones the
 * plan was created with.  `stream` overrides problem->stream.                            */
int smr_plan_execute(smr_plan* plan, void* const* bases, void* stream);
int smr_plan_destroy(smr_plan* plan);
/* Builds everything the first execution would build -- index tables uploaded, the kernel for a
 * runtime-compiled f compiled and loaded, reduction scratch allocated -- without launching.
 * Call it before capturing smr_plan_execute into a hipGraph (uploads are synchronous copies).  */
int smr_plan_prepare(smr_plan* plan);
/* Writes a one-line description ("family=tiled tile=32x32 grid=1024 ...") into buf.
 * family=contract (outer-product reductions, the box of the generic mul!: two inputs that vary along different kept
 * dims) reads "tile=d<i>:<TI>xd<j>:<TJ> k=<TK> grid=<G> lds=<bytes> vec=<V>": input tiles are staged in LDS once per
 * chunk of TK reduced elements and every lane keeps a block of outputs in registers (tiles of 64, 32 or 16 squared).
 * Its accumulation order is defined: one lane per output, from the operator's neutral element, over the outer reduced
 * index and then the inner reduced dim, ascending, the (init-ed) old destination combined last -- for real floats
 * bit-identical to the sequential loop.
 * Option "contract_split" (default 0 = never; negative: SMR_EINVAL) adds the SPLIT FORM, whose plans append
 * "kparts=<S> cps=<chunks per slice> fold=second-launch scratch=<bytes>": the chunk walk over (outer reduced index, k) is
 * cut into S contiguous, non-empty slices, one workgroup per (tile, slice) stores its block of accumulators as partials
 * (plan-owned scratch, allocated by the first execution or smr_plan_prepare), and a second launch folds every output's
 * partials in slice order and applies initop / the destination's type: dest = op(initop(old), op(...op(P_0, P_1)..., P_{S-1})),
 * P_s accumulated sequentially from the neutral element over slice s.  Run-to-run identical; for real floats bit-identical
 * to that loop, NOT to the unsplit one -- hence opt-in.  1 = by the planner's rule (problems whose unsplit plan has fewer
 * than 256 workgroups and a long reduced range); N >= 2 = N slices (clamped to the chunks) wherever a CONTRACT plan is made.
 * Option "contract_tile" (default 0 = the planner's rule; 16, 32 or 64; anything else: SMR_EINVAL) forces the tile of
 * single-call CONTRACT plans, split or not; a forced tile that does not fit "max_lds_bytes" refuses the family for the problem.
 * Contraction groups read neither option: their tile is "group_contract_tile" and their split form "group_contract_split"
 * (SPLIT CONTRACTION GROUPS below), whose slices are cut by the same arithmetic.                                         */
int smr_plan_describe(const smr_plan* plan, char* buf, size_t buflen);
/* Algorithmic bytes of one execution: every distinct operand footprint counted once
 * (SURVEY.md section 8d).                                                                 */
int64_t smr_plan_algorithmic_bytes(const smr_plan* plan);
/* Introspection of the TILED family's execution order (no reference counterpart: the
 * reference walks its blocks in loop order, src/mapreduce.jl:385-401).  Returns the number
 * of workgroups n of the launch, or 0 when tiles run in natural order; writes
 * min(n, cap) entries: out[b] = linear tile id executed by workgroup b, 0xffffffff = idle
 * padding.  Workgroup b runs on XCD b mod 8.
 * ORBIT family: a workgroup holds one tile per LDS slot (as many slots as the views' permutation group has elements, four for a
 * group of order three); the list has `slots` entries per workgroup (n = slots * grid, `grid` as smr_plan_describe prints it):
 * out[b * slots + g] = tile in slot g of workgroup b, the first of an idle workgroup is 0xffffffff.  Every tile of the box
 * appears exactly once, except that a group of order three repeats slot 0 in slot 3 and an incomplete last workgroup of
 * shared (diagonal) orbits repeats its slot 0.                                             */
int64_t smr_plan_tile_order(const smr_plan* plan, uint32_t* out, size_t cap);
/* ORBIT family, PAIR form (4^4 cubes of 8-byte elements, a group of order four; `pair_grid` in smr_plan_describe): the work list
 * the PAIR kernel walks -- EIGHT tiles per workgroup, out[w * 8 + b * 4 + g] = tile in slot g of the workgroup's slot set b
 * (the first of an idle workgroup is 0xffffffff).  Every tile of the box appears exactly once (an odd set out repeats set 0);
 * where the planner found it, set 1 is the orbit of set 0's unit-axis neighbour (tile + 1).  Returns the number of entries,
 * 0 when the plan has no PAIR form.  No reference counterpart.                                                            */
int64_t smr_plan_orbit_pairs(const smr_plan* plan, uint32_t* out, size_t cap);
/* Introspection of the two-sided FLAT form (no reference counterpart): the two memory runs a tile is the product of, for the
 * planner tests (tests/test_abi.py walks every tile with these numbers on the CPU and checks that each element of the box is
 * moved exactly once, from the right place to the right place).  Returns the number of values the description has -- 0 when the
 * plan is of another kind -- and writes min(that, cap) of them:
 *   [0] kt (operand index of the transposed input)   [1] shared   [2] N (canonical rank)
 *   [3..4] R[0], R[1]   [5..6] TP[0], TP[1]   [7..8] p[0], p[1] (-1: none)
 *   then N dims, N destination strides, N strides of operand kt, N flags ingroup[0], N flags ingroup[1],
 *   R[0] offsets roff[0][r], R[1] offsets roff[1][r]      (side 0 = destination, 1 = operand kt; canonical dim order) */
int64_t smr_plan_flat_runs(const smr_plan* plan, int64_t* out, size_t cap);
/* The same for the ONE-sided FLAT forms (plain, fused, shared-lead); 0 for any other plan.  Values:
 *   [0] dir (0: the destination is the flat side, 1: operand kt is)   [1] R   [2] tplog   [3] tqlog   [4] p   [5] q
 *   [6] lshare   [7] fuse   [8] kt   [9] N   then N dims, N destination strides, N strides of operand kt, N flags ingroup,
 *   R offsets roff[r] (line-side offset of leading index r of the flat run)                                                */
int64_t smr_plan_flat_side(const smr_plan* plan, int64_t* out, size_t cap);
/* The same for the BATCHED form (round 4: contiguous blocks on both sides, csrc/smr_k_flat.hip: flatb_body); 0 for any other plan:
 *   [0] g (dims of a block)   [1] P (elements of a block)   [2] K (blocks per workgroup)   [3] N
 *   then N dims, N destination strides, N input strides, P offsets srcoff[r] (input offset inside the block of destination position r) */
int64_t smr_plan_flat_batched(const smr_plan* plan, int64_t* out, size_t cap);

/* ---- grouped launches: many small independent maps -- or contractions -- as ONE kernel launch -----------
 * A launch cannot finish in under about 2 us on MI355X, so K small maps issued one by one cost K launches however little each
 * moves (the blocks of a block-sparse tensor contraction: permutedims!, axpby!, copy! on dozens to hundreds of sub-views of a few
 * parents).  A GROUP is K maps ("members") that run as one launch of one kernel (csrc/smr_k_group.hip): every workgroup finds its
 * member in a device table and runs it.  No reference counterpart (the reference spawns one task tree per call).
 * smr_group_create accepts the members when all of this holds; anything else that is valid returns SMR_EUNSUPPORTED with a message
 * naming the first offending member, malformed input SMR_EINVAL:
 *   - 1 <= count <= 65535, and every member is a valid map (redop == SMR_RED_NONE) -- or every member a contraction: the KIND of
 *     a group is member 0's, see "contraction groups" below; a map group refuses every reduction, a contraction group every map;
 *   - once canonicalised, all members compute in the same class, agree on whether they are bit copies and whether operand types
 *     are converted, have the same number M of distinct operands, the same dtype and conj flag per operand position and the same
 *     f-program including its constants: the kernel is instantiated once, f is ONE functor for the whole launch.  Members may
 *     differ in rank, dims, strides, base pointers and offsets;
 *   - with SMR_GROUP_MEMBER_SCALARS the VALUES of f's constants may differ as well (C_blk .= a_blk .* permutedims(A_blk, p) .+
 *     b_blk .* C_blk with a coefficient per block): the members still agree in everything above, in the program's length, every
 *     (opcode, immediate) pair, the number of constants and the functor f is recognised as.  A member whose constants put it into
 *     another compute class (a complex scalar among real ones, a non-integer scalar among integer arrays) is refused like any
 *     member of another class.  Every member keeps the constants of its own canonicalisation in a third device table (one row of
 *     doubles per member) that its workgroups read next to the descriptor; the kernel is still instantiated once, and a
 *     runtime-compiled f is compiled once for every set of scalars.  When all members' constants are bit-equal (-0.0 differs from
 *     0.0) the group is the one planned without the flag.  The scalars are fixed at creation, like the base pointers;
 *   - every member has at most 2^31 - 1 box elements;
 *   - independence: without SMR_GROUP_INDEPENDENT the bounding byte range [lo, hi) of a member's destination must not intersect
 *     the range of ANOTHER member's destination or inputs (the same ranges a recorded sequence compares); a member's destination
 *     may alias that member's own inputs under the rules of a single call.  With SMR_GROUP_INDEPENDENT the check is skipped and
 *     the CALLER asserts that no member writes an element another member reads or writes.  The flag is the only way to group
 *     interleaved blocks of one parent array, whose byte ranges overlap although their elements do not.
 * smr_group_create and smr_group_layout are host arithmetic only and need no device (like smr_plan_create).  smr_group_prepare
 * uploads the device tables and compiles + loads the kernel of a runtime-compiled f without launching; the first
 * smr_group_execute does the same when prepare was not called (the uploads are synchronous copies: prepare before capturing
 * an execute into a hipGraph).  smr_group_execute is ONE kernel launch, asynchronous on `stream` (NULL = the stream of member 0);
 * its result is bit-identical to smr_mapreduce on each member in order.  The launch goes through HIP; on a library-owned stream
 * (smr_stream_create) it is ordered behind the library's direct launches and the stream's next direct launch waits for it.  The base
 * pointers are fixed at creation (no rebinding).  A caller that executes the same group again and again records it into a sequence
 * (smr_seq_add_group): the replay is then one pre-built packet instead of one launch through HIP.
 * smr_group_describe: one line, "family=group members=K grid=G linear=a transposing=b f=<functor> jit=0/1 bytes=...", under
 * SMR_GROUP_MEMBER_SCALARS followed by " scalars=member" (a row of constants per member) or " scalars=shared" (they were equal).
 * smr_group_layout: per member 4 values -- form (0 linear, 1 transposing), first workgroup, workgroups, canonical rank; returns
 * 4 * count and writes min(that, cap) values.  The members' workgroup ranges tile [0, grid) in member order.
 *
 * CONTRACTION GROUPS.  When member 0 is a reduction the group is K outer-product reductions -- the generic mul! box
 * dest[i, j, rest] = op(initop(dest), op over k, q of f(in1[i, k, ..], in2[j, k, ..])) -- run as ONE launch of the grouped form of the
 * CONTRACT kernel (csrc/smr_k_gcontract.hip: LDS- and register-tiled; no partials, no scratch and no second launch unless option
 * "group_contract_split" splits a member, see SPLIT CONTRACTION GROUPS below).  Every member must
 * then be a reduction of that shape, whatever option "contract" says and whatever its size: once canonicalised it has exactly two
 * distinct inputs and no bit copy, at least two kept dims and one reduced dim, both inputs vary along the inner reduced dim, input 1
 * varies along a kept dim along which input 2 does not and the other way round, and neither input lies on the destination's buffer.
 * (Size-1 dims are dropped first: a member with m == 1 is not of the shape.)  A member that is not gets SMR_EUNSUPPORTED with
 * "contraction" in the message.  Every member must agree with member 0 in compute class, in whether operand types are converted,
 * in dtype and conj flag per operand position, in the f-program including its constants, in redop and in the initop CODE; initarg
 * (beta) is the member's own, and so are rank, extents, strides, pointers, offsets and batch / outer reduced dims.
 * SMR_GROUP_MEMBER_SCALARS with a contraction group is SMR_EUNSUPPORTED (per-member constants of f: not supported there).  A
 * contraction group takes them under a flag of its own, SMR_GROUP_CONTRACT_SCALARS: see PER-MEMBER CONSTANTS OF A CONTRACTION GROUP
 * below.  The
 * independence check (the destination's range is a write range, which covers the read of the old destination), the footprints, the
 * 2^31 - 1 workgroup limit and the count limits are those of map groups.
 * One tile size per group: 32 x 32 outputs per workgroup when the group then still has >= 256 workgroups and those tiles are at
 * least half full over the group, else 16 x 16; option "group_contract_tile" (16 / 32) forces it.  A tile that does not fit option
 * "max_lds_bytes" falls back to 16 x 16, and creation returns SMR_EUNSUPPORTED if that does not fit either.  A member's workgroups
 * are its tiles along the two tiled dims times its other kept extents, exactly what a single call's plan counts for that tile.
 * Accumulation order is the single call's: one lane per output, from the neutral element, over the outer reduced index ascending
 * and inside it over k ascending, the init-ed old destination combined last.  Each member's result is bit-identical to
 * smr_mapreduce on that member alone under option "contract" = 2, whatever tile either side picked.
 * smr_group_describe reads "family=group kind=contract members=K grid=G tile=<16|32> k=<chunk of the reduced dim> lds=<bytes>
 * f=<mul2|prog> op=<+|*|min|max|&||> jit=<0|1> bytes=<algorithmic bytes>[ independent=asserted]"; smr_group_layout reports form 2
 * for every member.  prepare, execute, destroy and smr_seq_add_group work as for map groups (a recorded contraction group is one
 * packet per replay and can be cut into block ranges).
 *
 * SPLIT CONTRACTION GROUPS.  Option "group_contract_split" (default 0; smr_group_create reads it for contraction groups only, like
 * "group_contract_tile") cuts long reduced ranges over workgroups: a few blocks with small open legs and a very long contracted leg
 * otherwise get a handful of workgroups.  0: never -- plans, describe(), layout() and launches are those of a library without the
 * option.  N >= 2: every member's walk over its Q * nkc chunks (nkc = ceil(K / k)) is cut into N slices by the single call's
 * arithmetic: N clamped to the chunks, cps = ceil(chunks / S), S = ceil(chunks / cps), no slice empty; a member left with one slice
 * is an unsplit member.  1: the group rule -- only for a group whose unsplit plan has fewer than 256 workgroups; "contract_split"'s
 * rule (slices of >= 2 chunks, <= 64 slices, the partials' round trip <= half the bytes the member's inputs move) bounds every
 * member's slices, the tile is the largest allowed one on which the members' tiles * bounds reach 256 (else the one that allows the
 * most), and with G the unsplit grid on it every member gets clamp(ceil(512 / G), 1, its bound) slices; a group in which no member
 * can take two slices is not split.  Negative values and values above 2^31 - 1 are SMR_EINVAL in smr_set_option; a forced N whose
 * slices need more than 2^31 - 1 workgroups is SMR_EINVAL and one whose partials exceed 2^31 bytes over the group SMR_EUNSUPPORTED
 * (naming the limit) in smr_group_create; under the rule such a group simply is not split.
 * A group with a split member is TWO launches.  Main launch: member i has tiles_i * S_i workgroups, the slice the slow digit; a
 * workgroup of a split member (S_i >= 2) accumulates its slice from the neutral element and stores its register block -- compute-
 * class values, no conversion, no conj, no initop; ragged tiles store all their lanes -- to the group's partials; a workgroup of an
 * unsplit member (S_i == 1) finishes its outputs in this launch as in an unsplit group (a thousand small blocks next to two long
 * ones do not go through the partials).  Fold launch: (tile / 16)^2 workgroups per tile of the split members only, one lane per
 * output folds P_0 .. P_{S-1} in slice order and applies the member's own initop argument; it does not call f (natively compiled
 * also when f is runtime-compiled).  ACCUMULATION ORDER of a split member: dest = op(initop(old), op(... op(P_0, P_1) ..., P_{S-1})),
 * P_s sequential from the neutral element over slice s.  A member with S_i >= 2 is bit-identical to smr_mapreduce on that member
 * alone under "contract" = 2, "contract_tile" = the group's tile and "contract_split" = S_i; a member with S_i == 1 is bit-identical
 * to the single call under "contract" = 2, as in an unsplit group.
 * The partials are owned by the group: smr_group_prepare or the first execution allocates them (sum over split members of tiles_i *
 * S_i * tile^2 * compute-class element size), smr_group_destroy frees them after draining the device.  ONE buffer per group: two
 * executions of one group in flight on different streams would share it -- that is the caller's problem, as for a split plan.  A run
 * writes every partial it reads: nothing depends on what an earlier run left there.
 * smr_group_describe appends " split=<members split> kparts=<max S_i> fold=second-launch fold_grid=<F> scratch=<bytes>" after
 * "bytes=..." (before " independent=asserted") when at least one member is split; grid= is the main launch's grid.
 * smr_group_layout stays at 4 values per member, "workgroups" being tiles_i * S_i.  smr_group_split_layout: per member 4 values --
 * S_i, cps_i, first fold workgroup, fold workgroups; returns 4 * count and writes min(that, cap) values; returns 0 for map groups
 * and groups without a split member.  smr_seq_add_group records a split group as its two launches inside ONE item (smr_seq_info still
 * counts one item and one group): the fold carries the barrier bit and acquires, like the second launch of a split CONTRACT plan;
 * the footprint other items are compared against stays the members' operands (the partials are private to the group).  Under
 * "slices" = n (smr_seq_set; never automatically) the main launch of a split group that is a component of its own is cut into n
 * block ranges of at least 64 workgroups each, like an unsplit group -- but the ranges go back to back onto the item's ONE queue and
 * the fold follows them with the barrier bit, so it runs after all of them (no order across queues exists): n + 1 packets.
 *
 * PER-MEMBER CONSTANTS OF A CONTRACTION GROUP.  SMR_GROUP_CONTRACT_SCALARS (contraction groups only; combines with
 * SMR_GROUP_INDEPENDENT) lets the VALUES of f's constants differ from member to member: mul!(C_blk, A_blk, B_blk, alpha_blk, beta_blk)
 * with a coefficient per block, f = x * y * alpha, is one group.  The members still agree with member 0 in everything listed above, in
 * the program's length, every (opcode, immediate) pair and the number of constants; a member whose constants put it into another
 * compute class is refused like any member of another class.  With SMR_GROUP_REDUCE, on a map group (member 0 is a map) or together
 * with SMR_GROUP_MEMBER_SCALARS the flag is SMR_EUNSUPPORTED, the message naming it.  Every member keeps the constants of its own
 * canonicalisation in a third device table, one row of W doubles per member (2 * the number of constants, (re, im) pairs), which
 * smr_group_prepare or the first execution uploads and smr_group_destroy frees after draining the device.  A workgroup reads the row
 * of ITS MEMBER -- not of its tile or slice: every tile and every slice of a member reads the same row -- by scalar loads, before
 * any data load.  When all rows are bit-equal (-0.0 differs from 0.0) the plan is the one planned without the flag, with no table.
 * Nothing else in the plan depends on the flag: tile rule, slices ("group_contract_split"), workgroups, layout and footprint are those
 * of the same members without it.  The program `arg1 arg2 MUL const MUL` -- the mul! form -- on operands of the compute class runs a
 * natively compiled functor in such a group (f=mul2scale, (a * b) * alpha with the f-program's own multiply: bit-equal to the
 * program); every other f with constants, and every group that converts operand types, is runtime-compiled or interpreted, and the
 * runtime-compiled text depends on the structure of f only: one code object for every table of constants.
 * GUARANTEE: member i is bit-identical to smr_mapreduce on that member alone, with its own constants, under "contract" = 2 (a split
 * member: also "contract_tile" = the group's tile and "contract_split" = S_i).  smr_group_describe appends " scalars=member" (a table)
 * or " scalars=shared" (the rows were equal) at the very end, and reads f=mul2scale jit=0 for the recognised product of a
 * scalars=member group.  A recorded scalars=member group is one packet per replay (two in one item when split) and is cut into block
 * ranges under "slices" like any contraction group: the kernel finds its member, and with it its row, from its index in the group.
 *
 * REDUCTION GROUPS.  With SMR_GROUP_REDUCE the group is K COMPLETE reductions -- a norm, an inner product, max |x| per block:
 * dest = op(initop(dest), op over the whole box of f(in1, in2, ...)) with a destination of ONE element -- run as ONE launch of
 * csrc/smr_k_greduce.hip.  Without the flag nothing changes: a reduction as member 0 still opens a contraction group.  Every member
 * must be a reduction (redop != SMR_RED_NONE) whose destination, once canonicalised, is one element, with 1 .. SMR_MAXM - 1 distinct
 * inputs and at most 2^31 - 1 box elements; a map, or a reduction that keeps a dim of extent > 1, gets SMR_EUNSUPPORTED naming the
 * member, with "complete" in the message.  Members agree with member 0 exactly as contraction members do (compute class, whether
 * operand types are converted, the number of distinct operands, dtype and conj flag per operand position, the f-program including
 * its constants, redop, the initop CODE); initarg (beta), rank, extents, strides, pointers and offsets are the member's own.
 * SMR_GROUP_REDUCE | SMR_GROUP_MEMBER_SCALARS is SMR_EUNSUPPORTED; SMR_GROUP_INDEPENDENT combines as usual.  The independence check,
 * the count limits, the footprints, prepare / execute / destroy / describe / layout and smr_seq_add_group work as for the other
 * kinds; the destination counts as READ in the footprint unless the initop code is ZERO or CONST.
 * Member i gets W_i = min(ceil(total_i / 4096), 64) workgroups of 256 lanes -- what a single call takes under option
 * "reduce_blocks" = 64 -- and the body the single call would take: the vector body (16-byte loads) when no operand type is converted,
 * a 16-byte vector holds more than one element of the compute class, the canonical rank is 1, total_i is a multiple of the vector
 * and at least 4096, and every input is broadcast or unit-stride from a 16-byte aligned address (the base pointers are fixed at
 * creation, so alignment is decided there); the strided body otherwise.
 * ACCUMULATION ORDER: that of the single call's complete-reduction kernel on a grid of W_i workgroups -- four accumulators per
 * lane (vector body: a wave reads 4 consecutive 1-KiB rows per iteration; strided body: a grid stride of W_i * 256 with 4 elements
 * in flight), the pairwise tree over the four, the wave butterfly, four wave sums through LDS.  W_i == 1: lane 0 applies the initop
 * with the member's beta, redop, and stores.  W_i > 1: every workgroup publishes its partial write-through into the member's run of
 * W_i slots, arrives at the member's counter, and the workgroup that arrives last folds the slots in slot order and stores -- inside
 * the same launch; nobody waits or polls.  GUARANTEE: member i's result is bit-identical to smr_mapreduce on that member alone under
 * option "reduce_blocks" = 64 whenever that call runs family REDUCE_ALL (the default of 2048 differs from 64 only above 64 * 4096
 * elements).  A single call hands a complete reduction of canonical rank > 1 whose inputs run along dim 0 (a sub-box) to the ROW form
 * of REDUCE_PART instead, which accumulates in another order; a group runs such a member on the strided body above.
 * The partials (compute-class elements, a contiguous run of W_i slots per member with W_i > 1) and the arrival counters (one per
 * such member) are owned by the group: smr_group_prepare or the first execution allocates them and ZEROES the counters, the last
 * arriver leaves its counter at zero for the next run, smr_group_destroy frees both after draining the device.  Two executions of
 * one group in flight at once share them: that is the caller's problem, as for split plans and split contraction groups.
 * smr_group_describe reads "family=group kind=reduce members=K grid=G vec=<members on the vector body> strided=<on the strided body>
 * f=<ident|abs2|mul2|prog> op=<+|*|min|max|&||> jit=<0|1> partials=<members with W > 1> scratch=<bytes> bytes=<algorithmic bytes>
 * [ independent=asserted]"; smr_group_layout reports form 3 (strided) or 4 (vector), the first workgroup, W_i and the canonical rank.
 * The launch is NOT sliceable -- the fold needs all of a member's workgroups in one launch: a recorded reduction group is one
 * packet per replay and stays whole under "slices" = n.  Option "nt_load" selects non-temporal loads in the vector body as in a
 * single call; it does not change values.
 *
 * PARTIAL REDUCTION GROUPS.  With SMR_GROUP_REDUCE | SMR_GROUP_REDUCE_PART the group is K reductions that may KEEP dims -- a
 * matrix-vector product y[i] = sum_j A[i,j] * x[j], row or column norms, a partial trace, sum(A; dims=2) per block:
 * dest[I] = op(initop(dest[I]), op over the reduced dims of f(in1, in2, ...)) with a destination that keeps any number of dims -- run
 * as ONE launch of csrc/smr_k_greduce_part.hip.  SMR_GROUP_REDUCE_PART without SMR_GROUP_REDUCE is SMR_EUNSUPPORTED; without the flag
 * every other combination plans, describes, launches and refuses exactly as before (flag 8 alone still refuses a kept dim with
 * "complete").  It combines with SMR_GROUP_INDEPENDENT and is refused with SMR_GROUP_MEMBER_SCALARS and SMR_GROUP_CONTRACT_SCALARS as a
 * reduction group refuses them.  Every member must be a reduction (redop != SMR_RED_NONE; a map gets SMR_EUNSUPPORTED naming the
 * member) with 1 .. SMR_MAXM - 1 distinct inputs and at most 2^31 - 1 box elements; members agree with member 0 exactly as in a
 * reduction group; beta, rank, extents, strides, pointers, offsets and WHICH dims are kept are the member's own.  Members with one
 * destination element and members with no reduced dim at all (the accumulating map dest[I] = op(dest[I], f(...))) are accepted.  The
 * independence check, the count limits, prepare / execute / destroy and smr_seq_add_group work as for the other kinds.  A member's
 * destination range in the check and in the footprint is its whole bounding range, so destinations that interleave in memory (the
 * columns of one matrix) need SMR_GROUP_INDEPENDENT; the destination counts as READ unless the initop code is ZERO or CONST.
 * RULE: member i takes the general form of a single partial reduction with the reduced range in ONE piece: TR_i consecutive lanes (a
 * power of two, 1 .. 256: what the single planner's general form gives that canonical problem) cooperate on one destination element, a
 * workgroup of 256 lanes owns 256 / TR_i consecutive destination elements in canonical order, W_i = ceil(nout_i / (256 / TR_i)).  The
 * group never splits a member's reduced range: no partials, no counters, no scratch -- long members are not what a group is for.
 * ACCUMULATION ORDER: with red_i reduced elements per destination element in canonical order, lane rl = 0 .. TR_i - 1 of a destination
 * element accumulates r = rl, rl + TR_i, rl + 2 TR_i, ... serially into one accumulator that starts at the op's neutral element; the
 * TR_i accumulators are folded by the wave butterfly (xor 32, 16, ... 1 below min(TR_i, 64)) and, for TR_i > 64, lane 0 then adds the
 * waves' values in ascending order through LDS; lane 0 applies the initop with the member's beta, the op, and stores.
 * GUARANTEE: member i's result is bit-identical to smr_mapreduce on that member alone under option "reduce_part_kind" = 0 wherever
 * that call's description reads "form=general lanes_per_out=TR_i split=1".  No identity is claimed for members the single planner would
 * split (red >= 256 * TR with few outputs), members with one destination element (a single call runs REDUCE_ALL) and members with no
 * reduced dim; their order is still the one above.
 * smr_group_describe reads "family=group kind=reduce_part members=K grid=G lanes=<TR:members, ascending TR, comma separated>
 * f=<ident|abs2|mul2|prog> op=<+|*|min|max|&||> jit=<0|1> bytes=<algorithmic bytes>[ independent=asserted]"; smr_group_layout reports
 * form 5, the first workgroup, W_i and the canonical rank; smr_group_lanes reports TR_i per member (layout has no room for it).
 * No workgroup depends on another, so the launch IS sliceable: a recorded partial reduction group is one packet per replay and is cut
 * into block ranges under "slices" = n, like a map group.                                                                        */
typedef struct smr_group smr_group;
#define SMR_GROUP_INDEPENDENT 1u /* the caller asserts that no member writes an element another member reads or writes */
#define SMR_GROUP_MEMBER_SCALARS 2u /* the values of f's constants may differ from member to member */
#define SMR_GROUP_REDUCE 8u /* a reduction group: every member a complete reduction (REDUCTION GROUPS above; bit 4 is not a flag) */
#define SMR_GROUP_CONTRACT_SCALARS 64u /* a contraction group whose members have constants of f of their own (bits 4, 16 and 32 are not flags) */
#define SMR_GROUP_REDUCE_PART 256u /* with SMR_GROUP_REDUCE only: the members may keep dims (PARTIAL REDUCTION GROUPS above; bit 128 is not a flag) */
int smr_group_create(const smr_problem* members, int count, uint32_t flags, smr_group** out);
int smr_group_prepare(smr_group* g);
int smr_group_execute(smr_group* g, void* stream);
int smr_group_describe(const smr_group* g, char* buf, size_t buflen);
/* Sum of the members' algorithmic bytes (smr_plan_algorithmic_bytes). */
int64_t smr_group_algorithmic_bytes(const smr_group* g);
int64_t smr_group_layout(const smr_group* g, int64_t* out, size_t cap);
int64_t smr_group_split_layout(const smr_group* g, int64_t* out, size_t cap);
/* A partial reduction group: the lanes per destination element TR_i of up to `cap` members into out[]; returns the member count (0 for
 * every other kind of group). */
int64_t smr_group_lanes(const smr_group* g, int64_t* out, size_t cap);
int smr_group_destroy(smr_group* g);

/* Runtime compilation.  An `f` without a natively compiled functor is specialised the way
 * Julia specialises the reference's @generated kernel per closure (src/mapreduce.jl:229-425):
 * the f-program is turned into a C++ functor and the plan's kernel is compiled for it with
 * hiprtc on first execution (cached per process; option "jit" = 0 keeps the bytecode
 * interpreter, which is also the fallback when hiprtc is unavailable).
 * smr_plan_jit_compile: generate + compile now, without a device (warms the compiler cache;
 * *code_size = bytes of the code object, 0 when the plan's kernel needs no compilation).
 * smr_plan_jit_source: the generated functor as text.                                     */
int smr_plan_jit_compile(smr_plan* plan, size_t* code_size);
int smr_plan_jit_source(const smr_plan* plan, char* buf, size_t buflen);

/* Block-partition a problem over `nshards` devices/ranks exactly like the reference's
 * task bisection splits the iteration box (src/mapreduce.jl:203-222): sub-box `shard`
 * gets its dims and per-operand offsets in *out.  Pure host arithmetic.  For reductions
 * whose split dim is a reduced one, *needs_allreduce is set: the caller combines the
 * per-shard partial destinations with RCCL (ncclAllReduce, op = redop).                  */
int smr_shard(const smr_problem* problem, int nshards, int shard, smr_problem* out,
              int* needs_allreduce);
/* The same with block-partitioned operands: bit k of `local_ops` says that ops[k].base/offset
 * already address THIS shard's slab (box index `start` of the split dim is the operand's index 0
 * along it; strides unchanged), so that operand's offset is not shifted and nothing has to be
 * replicated across devices.  *split_dim / *start / *stop (optional) report the slab
 * [start, stop) of box dim split_dim this shard owns (-1 when nshards == 1).               */
int smr_shard_ex(const smr_problem* problem, int nshards, int shard, uint32_t local_ops,
                 smr_problem* out, int* needs_allreduce, int* split_dim, int64_t* start,
                 int64_t* stop);
/* Writes the neutral element of problem->redop (0, 1, +inf, -inf, true, false) into every
 * distinct destination element: what _init_reduction! does for the per-task partial slots
 * (src/mapreduce.jl:182-191,157-163).  Asynchronous on problem->stream.                    */
int smr_init_reduction(const smr_problem* problem);

/* ---- multi-GPU from plain C: one process per GPU, RCCL over xGMI --------------------------
 * The C twin of what strided.jl_amd/distributed.py does through torch.distributed, for hosts
 * without it (the Julia shim).  Rank 0 calls smr_comm_unique_id and ships the 128 bytes to
 * the other ranks out of band (MPI, a socket, a file); every rank -- with its device already
 * selected (smr_init) -- calls smr_comm_init.  smr_mapreduce_sharded then executes ONE logical
 * problem cooperatively: every rank passes the same problem over its own device copies of
 * the operands; smr_shard picks this rank's sub-box; a split reduced dim is completed by one
 * ncclAllReduce of the destination elements (initop / old destination content enter once,
 * on rank 0: the distributed form of src/mapreduce.jl:153-170).  Map: on return each rank's
 * destination holds its own slab.  Reduce: every rank's destination holds the full result.
 * With nranks == 1 everything degenerates to smr_mapreduce and RCCL is never loaded.       */
int smr_comm_unique_id(void* out, size_t len);
int smr_comm_init(int nranks, int rank, const void* unique_id, size_t len);
/* (rank, nranks) as the COMMUNICATOR reports them (ncclCommUserRank / ncclCommCount); (0, 1) without one. */
int smr_comm_rank(int* rank, int* nranks);
/* Path of the RCCL library in use.  Choice: $SMR_RCCL_LIB when set; else a librccl the process has already
 * loaded (a host that ships its own, e.g. torch/lib/librccl.so: never two copies in one process); else the
 * system's librccl.so.1.                                                                                   */
int smr_comm_library(char* buf, size_t buflen);
int smr_comm_destroy(void);
int smr_mapreduce_sharded(const smr_problem* problem);
/* ... with block-partitioned operands (see smr_shard_ex).                                   */
int smr_mapreduce_sharded_ex(const smr_problem* problem, uint32_t local_ops);

/* Tuning knobs: the analogue of the reference's compile-time constants MINTHREADLENGTH /
 * BLOCKMEMORYSIZE (src/mapreduce.jl:141,462).  smr_set_option returns SMR_EINVAL for an unknown name and
 * clears the plan cache (except for the stamp buffer); smr_get_option returns -1 for an unknown name.
 * Defaults in parentheses; -1 usually means "the planner's rule".
 *   Families: "force_family" (0 auto, 1 generic, 3 tiled), "jit" (1: runtime compilation of f;
 *     0 interprets), "max_lds_bytes" (65536).
 *   TILED: "tile_log2" (0 auto, 10, 12), "tile_lg0".."tile_lg7" (-1: per-dim log2 tile extent),
 *     "tile_order" (1: orbit-major tile order for permuted views of one buffer), "tile_block" (-1: block
 *     tile order for distinct arrays with >= 3 unit axes; 0 off; n: blocks of n tiles per dim),
 *     "tile_block_xcd" (-1: one run of the block list per XCD while the operands fit the Infinity Cache;
 *     0 never; 1 always), "tiled_vec" (1: 16-byte accesses), "tiled_uavec" (1: ... at element
 *     alignment), "tiled_edge_first" (1: partly filled last tiles start first), "tiled_persist" (1) /
 *     "tiled_persist_wpc" (0 auto) / "tiled_persist_min" (32) (persistent pipelined form),
 *     "tiled_xpose" (1: lean kernel for HBM-sized transposing copies), "tiled_gorder" (-1: those copies
 *     walk the input's unit axis second; 0 canonical; 1 always).
 *   ORBIT: "orbit" (1: family on), "orbit_lg" (-1: log2 tile edge), "orbit_min" (150) / "orbit_few" (40)
 *     (orbit-count thresholds), "orbit_minrun" (16: shortest contiguous run in bytes), "orbit_group" (2:
 *     super-cell edge of the work list), "orbit_pipe" (-1: persistent pipelined form; 0 never; 1 always),
 *     "orbit_wgs" (0: cap on the workgroups of that form), "orbit_pair" (1: PAIR form of 4^4 cubes of
 *     8-byte elements), "orbit_pack" (1: orbits with fewer distinct tiles share a workgroup).
 *   FLAT: "flat" (1: family for short leading dims that are not powers of two), "flat_wide" (1: one-sided
 *     form for rows of 65..128 elements in matrices of >= 32 MiB; 2 wherever it applies), "flat2" (1:
 *     two-sided form; 0 off; 2 wherever it applies), "flat2_pair" (1), "flat2_bytes" (384),
 *     "flat2_lead_bytes" (512), "flat2_long" (80: two-sided form for long unit-stride dims whose 32 x 32
 *     tiles would be less full than this per cent; 0 off), "flatb" (1: batched form for small contiguous
 *     blocks).
 *   CONTRACT: "contract" (1: the LDS- and register-tiled family for reductions of two inputs that vary along
 *     different kept dims -- the generic mul! box -- when the problem is large enough: op = +, tile extents >= 32, at
 *     least 256 output tiles, an inner reduced dim of >= 16, and no f that "jit" = 0 would leave to the interpreter;
 *     0 never; 2 wherever the shape qualifies: tests and experiments).
 *   STREAM: "stream_ua" (1: element-aligned 16-byte vectors + a partial vector per row),
 *     "stream_pack_rows" (1: short rows share a workgroup), "nt_store" (-1: non-temporal stores; 0 never;
 *     1 always; 2 write-through), "nt_stream_min" (0).
 *   Reductions: "reduce_blocks" (2048), "reduce_part_wgs" (1024: partial reductions with fewer workgroups
 *     are split until about this many run), "reduce_part_kind" (-1; 0 general, 1 row, 2 col),
 *     "reduce_single" (4: split reductions of at most this many chunks fold their partials inside the same
 *     launch; 0 = always a second launch; a plan that owns partials must not run concurrently with itself
 *     on two streams), "reduce_row_floor" (-1), "reduce_row_dense" (1), "reduce_col_txlog" (5),
 *     "reduce_col_exact" (1), "reduce_col_narrow" (1), "nt_load" (-1: non-temporal loads of complete
 *     reductions; 0 never; 1 always).
 *   Dispatch: "eager_direct" (1: library-owned streams submit launches themselves), "seq_self_release"
 *     (1: launches recorded for a sequence issue agent-scope write-through stores where the family can and
 *     their packets carry no release fence), "eager_self_release" (1: the same on library-owned streams),
 *     "self_release_max_bytes" (64 MiB: largest destination for which that is done),
 *     "self_release_max_total" (128 MiB: largest footprint of a whole sequence / of the recently written
 *     destinations).
 *   Sharding: "allreduce_f64" (0; 1: Float32 / ComplexF32 sums cross the ranks as Float64).
 *   Groups: "group_max_bytes" (16 MiB: largest member, in algorithmic bytes, that a front end still defers into a group; read by the
 *     front ends only: setting it keeps the plan cache); "group_contract_tile" (0: the rule; 16 / 32 force the tile of contraction
 *     groups created afterwards: tests and measurements); "group_contract_split" (0: never; 1: the group rule; N >= 2: N slices
 *     per member of contraction groups created afterwards; negative or above 2^31 - 1: SMR_EINVAL; keeps the plan cache).
 *   Debug builds with device-side wall-clock stamps (csrc/smr_device.h): "stamp_base" / "stamp_cap" /
 *     "stamp_used"; read-only "stamp_build".
 *   Read-only counters: "launches" (kernel launches the library issued, through HIP or directly),
 *     "jit_compiles", "jit_hits", "jit_failures", "jit_compile_ms", "eager_launches", "eager_free" /
 *     "eager_same" / "eager_cross" (direct launches; executions that conflicted with nothing / one queue /
 *     several), "eager_fallback" (executions sent through HIP), "eager_kernarg_device", "eager_arg_hits",
 *     "eager_gpu_only_signals", "allreduces", "allreduces_inplace".
 * Environment: $SMR_DIRECT_TIMEOUT_MS (30000: no-progress limit of waits on the direct queues),
 * $SMR_DIRECT_SELFTEST (0 skips, "fail" forces the failure path), $SMR_DIRECT_METADATA (0: code-object-v5 rule instead of the
 * metadata), $SMR_SEQ_DIRECT (0: sequences replay through HIP), $SMR_SEQ_STREAM_WAIT (1: hipStreamWaitValue64 where supported),
 * $SMR_RCCL_LIB (which collective library to dlopen).      */
int smr_set_option(const char* name, int64_t value);
int64_t smr_get_option(const char* name);

#ifdef __cplusplus
}
#endif
#endif /* STRIDED_HIP_H */
