"""Diffusion algorithms: sqrt schedule, DDIM / cold samplers, img2img, inpainting."""
from .schedule import (alpha_bar_train, cold_steps, ddim_coefficients, ddim_table, ddim_timesteps, dpm2m_row,
                       dpm2m_table, img2img_alpha, repaint_row, repaint_table)
from .samplers import ColdSampler, DDIMSampler, img2img, inpaint

__all__ = ["alpha_bar_train", "cold_steps", "ddim_coefficients", "ddim_table", "ddim_timesteps", "dpm2m_row",
           "dpm2m_table", "img2img_alpha", "repaint_row", "repaint_table", "ColdSampler", "DDIMSampler", "img2img",
           "inpaint"]
