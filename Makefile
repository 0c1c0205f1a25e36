# Builds the C-ABI HIP library (gfx950 only) and the C oracle helpers.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
CSRC  := medmoe_amd/csrc
SRCS  := $(wildcard $(CSRC)/*.hip)
OBJS  := $(patsubst $(CSRC)/%.hip,build/%.o,$(SRCS))
LIB   := medmoe_amd/lib/libmedmoe_hip.so
FLAGS := --offload-arch=$(ARCH) -O3 -fPIC -std=c++17 -Iinclude -I$(CSRC) -Wno-unused-result

all: $(LIB)

build/%.o: $(CSRC)/%.hip $(wildcard $(CSRC)/*.h)
	@mkdir -p build
	$(HIPCC) $(FLAGS) -c $< -o $@

$(LIB): $(OBJS)
	@mkdir -p medmoe_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS)

# host-only check of the staged wgrad plans (det_plan.h: range enumeration, slots, scratch sizes) under the sanitizers
CXX ?= c++
check-plan: tools/det_plan_check.cpp $(CSRC)/det_plan.h
	@mkdir -p build
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I$(CSRC) $< -o build/det_plan_check
	build/det_plan_check

# host-only model of the per-block row-sum exchange of the backward pair launch (pair3.hip), under the thread sanitizer
check-exchange: tools/pair3_exchange_check.cpp
	@mkdir -p build
	$(CXX) -std=c++17 -O1 -g -fsanitize=thread -pthread $< -o build/pair3_exchange_check
	build/pair3_exchange_check

# host-only check of the top-K list insert / merge (topk_list.h, shared with retrieval.hip) against std::stable_sort, under the sanitizers
check-topk: tools/topk_list_check.cpp $(CSRC)/topk_list.h
	@mkdir -p build
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I$(CSRC) $< -o build/topk_list_check
	build/topk_list_check

# host-only check of the LAMB record enumeration (lamb_plan.h, shared with lamb.hip): random segment tables, under the sanitizers
check-lamb-plan: tools/lamb_plan_check.cpp $(CSRC)/lamb_plan.h
	@mkdir -p build
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I$(CSRC) $< -o build/lamb_plan_check
	build/lamb_plan_check

# host-only check of the upsample supports of the segmentation head (seg_plan.h, shared with segment.hip): for random (g, H) the supports
# partition the (pixel, corner) pairs of non-zero weight and gather equals scatter in exact integers, under the sanitizers
check-seg-plan: tools/seg_plan_check.cpp $(CSRC)/seg_plan.h
	@mkdir -p build
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I$(CSRC) $< -o build/seg_plan_check
	build/seg_plan_check

clean:
	rm -rf build $(LIB)

.PHONY: all clean check-plan check-exchange check-topk check-lamb-plan check-seg-plan
