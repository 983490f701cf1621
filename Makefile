# Build the C-ABI HIP library (cross-compiles for gfx950 without a GPU).  One object per source so that a
# kernel edit recompiles one file; `make -j` compiles them in parallel.
HIPCC ?= hipcc
ARCH  ?= gfx950
CSRC  := $(wildcard srl_amd/csrc/*.hip)
HDRS  := $(wildcard srl_amd/csrc/*.h) include/srl_hip.h
OBJD  := srl_amd/csrc/build
OBJS  := $(patsubst srl_amd/csrc/%.hip,$(OBJD)/%.o,$(CSRC))
LIB   := srl_amd/csrc/libsrlhip.so
FLAGS := -O3 --offload-arch=$(ARCH) -std=c++17 -fPIC

all: $(LIB)

# rnn_wseq.hip (beside rnn_seq.hip in the wildcard above) keeps W_hh in registers: the build prints what each of its kernels
# took (registers, scratch -- which must be 0), and its cell arithmetic beside the MFMAs stays on unpacked float32 ops.
$(OBJD)/rnn_wseq.o: FLAGS += -Xclang -target-feature -Xclang -packed-fp32-ops -Rpass-analysis=kernel-resource-usage

# ln_heads_wide.hip likewise: head weights and their gradient sums resident in registers beside the MFMAs, no scratch.
$(OBJD)/ln_heads_wide.o: FLAGS += -Xclang -target-feature -Xclang -packed-fp32-ops -Rpass-analysis=kernel-resource-usage

# attn_xl.hip: a wavefront holds the whole 32 x F score strip (up to 6 accumulator blocks) beside its fragments, no scratch.
$(OBJD)/attn_xl.o: FLAGS += -Rpass-analysis=kernel-resource-usage

# gtrxl_gate.hip: six accumulator blocks (two-level sums) beside two weight fragments within 256 registers a lane, no scratch.
$(OBJD)/gtrxl_gate.o: FLAGS += -Rpass-analysis=kernel-resource-usage

# gtrxl_qkv.hip: six accumulator blocks forward, four backward beside sixteen registers of xhat, no scratch.
$(OBJD)/gtrxl_qkv.o: FLAGS += -Rpass-analysis=kernel-resource-usage

$(OBJD)/%.o: srl_amd/csrc/%.hip $(HDRS)
	@mkdir -p $(OBJD)
	$(HIPCC) $(FLAGS) -c -o $@ $<

$(LIB): $(OBJS)
	$(HIPCC) $(FLAGS) -shared -o $@ $(OBJS)

clean:
	rm -rf $(LIB) $(OBJD)

.PHONY: all clean
