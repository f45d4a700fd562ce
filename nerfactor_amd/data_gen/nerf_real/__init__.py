"""data_gen.nerf_real — a real capture (LLFF poses_bounds.npy and photographs) into the directory the NeRF stage reads (reference: data_gen/nerf_real/)."""
