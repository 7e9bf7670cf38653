!  qn_shift_draw_dev -- qn_shift_dev's loop (the reference's test/driver2.f90:66-195 on device buffers, the library's
!  built-in separable bounded quadratic, classic entry setulb_dev) to a NEW_X return, then the Laplace posterior on the
!  free variables under a Gaussian prior of precision MU = 0.5: the rows that lbfgsb_kkt reports at a bound (codes 1,
!  2, 3) are pinned (d_i = +inf), the others get d_i = 0 (lbfgsb_qn_shift_set with mu = 0.5).  Two draws from
!  N(0, (B + mu I + D)^-1) with their log-densities (lbfgsb_qn_shift_draw_logpdf: seed 1, samples 0 and 1, no mean,
!  scale 1), the log-densities and quadratic forms of the stored draws by the other route (lbfgsb_qn_shift_logpdf,
!  lbfgsb_qn_shift_quad), and L v for v = 1 (lbfgsb_qn_shift_sqrt).
!
!     qn_shift_draw_dev [n [m [iterations]]]      defaults 100000, 5, 12
!
!  Output: one "Iterate" line per iterate, then
!     QNSHIFTDRAW col = <stored pairs> pinned = <pinned rows>
!     QNSHIFTDRAW logp <log-density of draw 1> <of draw 2>          (from z, lbfgsb_qn_shift_draw_logpdf)
!     QNSHIFTDRAW logq <log-density of draw 1> <of draw 2>          (the quadratic form, lbfgsb_qn_shift_logpdf)
!     QNSHIFTDRAW quad <quadratic form of draw 1> <of draw 2>
!     QNSHIFTDRAW norms <|draw 1|> <|L v|> <largest |draw| or |L v| on a pinned row>
      program qn_shift_draw_dev

      use lbfgsb_module, wp => lbfgsp_wp
      use iso_c_binding
      use iso_fortran_env, only: output_unit
      use, intrinsic :: ieee_arithmetic, only: ieee_value, ieee_positive_inf

      implicit none

      interface
         function hipMalloc(ptr, nbytes) bind(C, name='hipMalloc') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr) :: ptr
            integer(c_size_t), value :: nbytes
            integer(c_int) :: rc
         end function hipMalloc
         function hipFree(ptr) bind(C, name='hipFree') result(rc)
            import :: c_ptr, c_int
            type(c_ptr), value :: ptr
            integer(c_int) :: rc
         end function hipFree
         function hipMemcpy(dst, src, nbytes, kind) bind(C, name='hipMemcpy') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr), value :: dst, src
            integer(c_size_t), value :: nbytes
            integer(c_int), value :: kind
            integer(c_int) :: rc
         end function hipMemcpy
         function hipMemset(dst, val, nbytes) bind(C, name='hipMemset') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr), value :: dst
            integer(c_int), value :: val
            integer(c_size_t), value :: nbytes
            integer(c_int) :: rc
         end function hipMemset
      end interface
      integer(c_int), parameter :: H2D = 1, D2H = 2

      integer               :: n, m, maxit, rc, i
      real(wp), parameter   :: factr = 0.0_wp, pgtol = 0.0_wp
      character(len=60)     :: task, csave
      character(len=32)     :: arg
      logical               :: lsave(4)
      integer               :: isave(44)
      real(wp)              :: f, dsave(29)
      real(c_double)        :: lp(2), lq(2), qq(2), s1, s2, xpin
      real(c_double), parameter :: MU = 0.5_c_double
      type(c_ptr)           :: ctx, dx, dg, dl, du, dnbd, du1, ddr, dd, dstatus
      real(wp), allocatable, target :: hu(:), hd(:), hdr(:)
      integer(c_int8_t), allocatable, target :: hstatus(:)
      integer(c_int64_t)    :: cnt(LBFGSB_KKT_NCNT), pinned
      real(c_double)        :: val(LBFGSB_KKT_NVAL)
      real(wp), allocatable, target :: hbuf(:)
      integer(c_int32_t), allocatable, target :: hnbd(:)
      integer(c_size_t)     :: vbytes

      n = 100000; m = 5; maxit = 12
      if (command_argument_count() >= 1) then
         call get_command_argument(1, arg); read (arg, *) n
      end if
      if (command_argument_count() >= 2) then
         call get_command_argument(2, arg); read (arg, *) m
      end if
      if (command_argument_count() >= 3) then
         call get_command_argument(3, arg); read (arg, *) maxit
      end if

      vbytes = int(n, c_size_t)*int(storage_size(1.0_wp)/8, c_size_t)
      call chk(hipMalloc(dx, vbytes), 'hipMalloc x')
      call chk(hipMalloc(dg, vbytes), 'hipMalloc g')
      call chk(hipMalloc(dl, vbytes), 'hipMalloc l')
      call chk(hipMalloc(du, vbytes), 'hipMalloc u')
      call chk(hipMalloc(du1, vbytes), 'hipMalloc u')
      call chk(hipMalloc(ddr, 2*vbytes), 'hipMalloc draws')
      call chk(hipMalloc(dd, vbytes), 'hipMalloc d')
      call chk(hipMalloc(dstatus, int(n, c_size_t)), 'hipMalloc status')
      call chk(hipMalloc(dnbd, int(n, c_size_t)*4_c_size_t), 'hipMalloc nbd')
      call chk(hipMemset(dx, 0_c_int, vbytes), 'hipMemset x')             ! x0 = 0
      call chk(hipMemset(dg, 0_c_int, vbytes), 'hipMemset g')
      allocate (hbuf(n))
      hbuf = -1.0_wp                                                       ! l = -1
      call chk(hipMemcpy(dl, c_loc(hbuf), vbytes, H2D), 'hipMemcpy l')
      hbuf = 1.0_wp                                                        ! u = +1
      call chk(hipMemcpy(du, c_loc(hbuf), vbytes, H2D), 'hipMemcpy u')
      allocate (hnbd(n))
      do i = 1, n
         hnbd(i) = int(mod(i, 4), c_int32_t)                               ! all four bound types
      end do
      call chk(hipMemcpy(dnbd, c_loc(hnbd), int(n, c_size_t)*4_c_size_t, H2D), 'hipMemcpy nbd')
      deallocate (hnbd)

      call lbfgsb_create(ctx, n, m, 0, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_create failed: ', lbfgsb_error_message()
         error stop 1
      end if

      task = 'START'
      f = 0.0_wp
      do while (task(1:2) == 'FG' .or. task == 'NEW_X' .or. task == 'START')
         call setulb_dev(ctx, dx, dl, du, dnbd, f, dg, factr, pgtol, task, -1, csave, lsave, isave, dsave, rc)
         if (rc /= 0) then
            write (output_unit, '(2a)') ' setulb_dev failed: ', lbfgsb_error_message()
            error stop 1
         end if
         if (task(1:2) == 'FG') then
            call lbfgsb_objective(ctx, 0, dx, dg, rc, f)
            if (rc /= 0) error stop 2
         else if (task(1:5) == 'NEW_X') then
            write (output_unit, '(2(a,i5,4x),a,1p,d12.5,4x,a,1p,d12.5)') 'Iterate', isave(30), 'nfg =', isave(34), &
               'f =', f, '|proj g| =', dsave(13)
            if (isave(30) >= maxit) exit                                   ! the model of this NEW_X return
         end if
      end do

      ! the rows at a bound at this iterate (codes 1, 2, 3 of lbfgsb_kkt's status) are pinned, the others not shifted
      call lbfgsb_kkt(ctx, dx, dl, du, dnbd, dg, 0.0_c_double, c_null_ptr, c_null_ptr, dstatus, cnt, val, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_kkt failed: ', lbfgsb_error_message()
         error stop 1
      end if
      allocate (hstatus(n), hd(n), hu(n))
      call chk(hipMemcpy(c_loc(hstatus), dstatus, int(n, c_size_t), D2H), 'hipMemcpy status')
      do i = 1, n
         if (hstatus(i) >= 1_c_int8_t) then
            hd(i) = ieee_value(1.0_wp, ieee_positive_inf)
         else
            hd(i) = 0.0_wp
         end if
      end do
      call chk(hipMemcpy(dd, c_loc(hd), vbytes, H2D), 'hipMemcpy d')
      call lbfgsb_qn_shift_set(ctx, dd, MU, pinned, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_qn_shift_set failed: ', lbfgsb_error_message()
         error stop 1
      end if
      write (output_unit, '(a,i4,a,i0)') 'QNSHIFTDRAW col =', isave(28), ' pinned = ', pinned
      ! two draws with their densities, then the densities and quadratic forms of the stored draws
      call lbfgsb_qn_shift_draw_logpdf(ctx, 2, 1_c_int64_t, 0, c_null_ptr, 1.0_c_double, ddr, n, lp, rc)
      if (rc == 0) call lbfgsb_qn_shift_logpdf(ctx, 2, ddr, n, c_null_ptr, 1.0_c_double, lq, rc)
      if (rc == 0) call lbfgsb_qn_shift_quad(ctx, 2, ddr, n, c_null_ptr, qq, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_qn_shift_draw_logpdf / _logpdf / _quad failed: ', lbfgsb_error_message()
         error stop 1
      end if
      write (output_unit, '(a,2es25.16e3)') 'QNSHIFTDRAW logp', lp(1), lp(2)
      write (output_unit, '(a,2es25.16e3)') 'QNSHIFTDRAW logq', lq(1), lq(2)
      write (output_unit, '(a,2es25.16e3)') 'QNSHIFTDRAW quad', qq(1), qq(2)
      ! L v for v = 1
      hbuf = 1.0_wp
      call chk(hipMemcpy(du, c_loc(hbuf), vbytes, H2D), 'hipMemcpy v')
      call lbfgsb_qn_shift_sqrt(ctx, 1, du, n, du1, n, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_qn_shift_sqrt failed: ', lbfgsb_error_message()
         error stop 1
      end if
      allocate (hdr(n))
      call chk(hipMemcpy(c_loc(hu), du1, vbytes, D2H), 'hipMemcpy L v')
      call chk(hipMemcpy(c_loc(hdr), ddr, vbytes, D2H), 'hipMemcpy draw 1')
      s1 = 0.0_c_double; s2 = 0.0_c_double; xpin = 0.0_c_double
      do i = 1, n
         s1 = s1 + real(hdr(i), c_double)**2
         s2 = s2 + real(hu(i), c_double)**2
         if (hstatus(i) >= 1_c_int8_t) xpin = max(xpin, abs(real(hdr(i), c_double)), abs(real(hu(i), c_double)))
      end do
      write (output_unit, '(a,3es25.16e3)') 'QNSHIFTDRAW norms', sqrt(s1), sqrt(s2), xpin
      deallocate (hstatus, hd, hu, hdr)

      task = 'STOP: QN_SHIFT_DRAW_DEV'
      call lbfgsb_destroy(ctx)
      rc = hipFree(dx); rc = hipFree(dg); rc = hipFree(dl); rc = hipFree(du)
      rc = hipFree(du1); rc = hipFree(dnbd); rc = hipFree(ddr); rc = hipFree(dd); rc = hipFree(dstatus)

      contains

      subroutine chk(code, what)
      integer(c_int), intent(in) :: code
      character(len=*), intent(in) :: what
      if (code /= 0) then
         write (output_unit, '(3a,i0)') ' ', what, ' failed, hipError ', code
         error stop 3
      end if
      end subroutine chk

      end program qn_shift_draw_dev
