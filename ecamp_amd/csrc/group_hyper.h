// The grouped optimizer launches over a flat parameter buffer (ecamp_adamw_grouped, optim.hip; ecamp_sgd_grouped, finetune.hip): parameters
// are padded to 64-element blocks, `block_group[i]` (uint8) names the param_group of block i (255 = frozen / unused -> skipped), and each
// group carries its own (lr, weight_decay).
#pragma once

struct GroupHyper {
    float lr[8];
    float wd[8];
};

constexpr int GROUPED_MAX_GRID = 8192;  // workgroups of a grouped launch: beyond it a thread takes several 16-byte vectors in turn
