// StarkConfig's FRI / MMCS parameters (vgpu_config_t): host-only, shared by the prover (pcs.hpp) and the verifiers (machine_verifier.hpp).
#pragma once

namespace vhost {

struct FriParams {
    unsigned log_blowup = 1, num_queries = 40, pow_bits = 8;
    bool observe_final_poly = false;
    bool interpret_air = false;  // quotient: force the register-program interpreter even for the in-tree chips
    int hash_kind = 0;           // MMCS hash: 0 Keccak-256 (reference), 1 Poseidon-16 sponge / truncated permutation (north-star variant)
};

}  // namespace vhost
