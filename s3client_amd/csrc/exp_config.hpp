// exp_config.hpp -- the compile-time switches of the kernels that something committed still
// builds with, in one place, with the values the PRODUCT build uses.  A switch lives here only
// while a Makefile target, a test or a tool under tools/ builds with it; an experiment that has
// been decided leaves its result in DESIGN.md and its code is deleted, not switched off
// (tests/test_code_object.py checks that the names used in the sources and the names below
// are the same set).
//
// Builds that may override what is below define S3H_EXPERIMENT_BUILD: the test-only
// forced-fault build (`make stall`) and experiment builds (`make exp TAG=...
// EXPFLAGS="-DS3H_EXP_..."`, timing studies under tools/exp/, never shipped).  Without it --
// the build of s3client_amd/lib/libs3hash.so -- every value switch must hold its default and
// no flag switch may be defined: the static_asserts and the #error below stop a product build
// that was compiled with such flags, so the shipped kernels are exactly the ones the
// measurements in DESIGN.md and the code hashes in kernel_isa_counts.json describe.
#pragma once

// ---- value switches: product defaults
#ifndef S3H_EXP_SHA1_BPS
// SHA-1 producer/consumer kernel: blocks per producer step while the grid fits one workgroup
// per CU (40 KiB of LDS per block of the step); 1: the 1-block form for every grid
// (tools/sha1_bench.py --exp-lib)
#define S3H_EXP_SHA1_BPS 2
#endif
#ifndef S3H_EXP_SPIN_LIMIT
#define S3H_EXP_SPIN_LIMIT (1u << 24)  // flag waits: s_sleep 1 polls before a wait times out
#endif
#ifndef S3H_EXP_STALL_PRODUCER
// 1: flag-synchronised producers stop publishing after their first step, so every consumer
// wait times out (the forced-fault build `make stall`, tests/test_gpu_errors.py)
#define S3H_EXP_STALL_PRODUCER 0
#endif

// ---- flag switches: the entry hooks of the generators under tools/
//   S3H_EXP_PRODUCER_INC  another generated skew producer instead of sha256_producer_simple.inc
//                         (tools/gen_producer.py), S3H_PROD_ZYV with its --zyv forms
//   S3H_EXP_MD5_INC       another generated MD5 step instead of md5_step_asm.inc
//                         (tools/gen_md5.py), S3H_MD5_VMEM with its vmem form

#ifndef S3H_EXPERIMENT_BUILD
static_assert(S3H_EXP_SHA1_BPS == 2, "product build: SHA-1 kernel with 2-block producer steps");
static_assert(S3H_EXP_SPIN_LIMIT == (1u << 24), "product build: flag waits give up after 2^24 polls");
static_assert(S3H_EXP_STALL_PRODUCER == 0, "product build: producers publish every step");
#if defined(S3H_EXP_PRODUCER_INC) || defined(S3H_PROD_ZYV) || defined(S3H_EXP_MD5_INC) || \
    defined(S3H_MD5_VMEM)
#error "an experiment switch is defined in a product build (define S3H_EXPERIMENT_BUILD: make exp)"
#endif
#endif  // S3H_EXPERIMENT_BUILD
