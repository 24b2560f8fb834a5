// digest.hpp — every digest's kernel family (merkle.hpp, blake2s.hpp, blake3.hpp, keccak.hpp) and the ONE place where a context's ms_digest_id becomes one of them.
#pragma once
#include "../../include/ministark.h"
#include "blake2s.hpp"
#include "blake3.hpp"
#include "keccak.hpp"

namespace msmerkle {

// f(family) for the kernel family of `digest` (an ms_digest_id; a context holds no other value: session.cpp decodes the MS_FLAG_DIGEST_* flags).  `f` is a generic
// callable that returns the same type for every family; what it launches is instantiated for all of them.  A family (the DG of LeafHashKernel and of
// msfri::FriTailKernel) names its Stream and the stream's constants, and its inner kernels Inner, Inner2 and Subtree; Blake3Kernels also names the multi-chunk
// instances and the bounds the host picks them by.
template <class Fn> inline auto with_digest(int digest, Fn&& f) {
  switch (digest) {
    case MS_DIGEST_BLAKE2S256: return f(Blake2sKernels());
    case MS_DIGEST_BLAKE3: return f(Blake3Kernels());
    case MS_DIGEST_KECCAK256: return f(Keccak256Kernels());
    case MS_DIGEST_SHA3_256: return f(Sha3_256Kernels());
    default: return f(Sha256Kernels());
  }
}

}  // namespace msmerkle
